/*
 * anirec.h — C ABI of libanirec.so, the MI355X (gfx950) kernel library behind the
 * anime_recommendations hot path.
 *
 * The reference (Dyrutter/anime_recommendations) is pure Python; its "plugin API" for
 * this path is the MLflow component surface (neural_network, similar_anime,
 * similar_users, model_recs) and the arithmetic lives in TensorFlow/Keras 2.12 and
 * NumPy calls made from those components.  Every entry point below replaces one such
 * call site (cited as reference file:line).  A maintainer of the reference would bind
 * them with ctypes (INTEGRATION.md shows the stubs).
 *
 * Conventions
 *  - extern "C", plain pointers + sizes, no C++/torch types.
 *  - every pointer is a DEVICE pointer unless the name ends in _host.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *  - return value: 0 = ok, negative = ANIREC_E*, positive = hipError_t.
 *  - the library never allocates device memory and never synchronises the stream
 *    (exception: the *_create/_destroy calls, which touch no stream work);
 *    all work is stream-ordered and graph-capturable.
 *  - apart from the training `workspace`, `rowmap` and `lazy_state` (zero before first use), no buffer needs any
 *    particular content on entry: a workspace may hold the leftovers of any earlier call.  Every output element in
 *    the documented extent is written, padding included.  Count and flag words (*n_out, *n_unique, out_max2,
 *    *err_flag, the flags arrays) are overwritten by the call: the caller need not clear them.
 *  - embedding rows are fp32, row-major, exactly ANIREC_DIM (=128) wide
 *    (reference: config/config.yaml:63 embedding_size: 128) — for every entry point without a `dim` argument.
 *  - OTHER WIDTHS (the reference's --embedding_size, neural_network.py:75-85): an entry point whose work depends on the
 *    row width has a twin NAME_w with an added `int32_t dim`; rows are then `dim` floats wide, dim in {32, 64, 128,
 *    256} — a row is dim / 4 lanes of float4, the 8-, 16-, 32- and 64-lane groups of a 64-lane wave.  Any other dim:
 *    ANIREC_EINVAL (0 from a *_bytes_w function) before anything is enqueued or written.  NAME(...) is
 *    NAME_w(..., ANIREC_DIM): same kernels, same results.  Wherever a comment below says [rows][128], read
 *    [rows][dim] for the twin.  128 only (no twin): the MFMA paths (*_mfma, anirec_cosine_topk_job), the lazy dense
 *    Adam (a descriptor with lazy != 0 and dim != 128 is ANIREC_EINVAL), the multi-GPU calls (anirec_dist_*,
 *    anirec_train_adam_part, dense_mode 1 and 2, n_seg > 1: ANIREC_EINVAL at another width) and
 *    anirec_train_stage_ticks.
 */
#ifndef ANIREC_H
#define ANIREC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANIREC_ABI_VERSION 5
#define ANIREC_DIM 128          /* embedding width (floats) */
#define ANIREC_MAX_BATCH 16384  /* ratings per rank per step handled by one sort workgroup */
#define ANIREC_CHUNK 32         /* max gradient contributions summed by one half-wave */
#define ANIREC_ADAM_BLOCKS 8192 /* grid of the dense Adam kernel == length of reg partials */
#define ANIREC_MAX_TOPK 128     /* k limit of the fused top-k kernels */
#define ANIREC_MAX_SEG 16       /* max head packets (ranks of one node) */
#define ANIREC_TOPK_MAX_BATCHES 64 /* query batches of one anirec_cosine_topk_job */
#define ANIREC_LAZY_WINDOW 8    /* steps between two flushes of the lazy dense Adam (anirec_trainer_run) */
#define ANIREC_FOLD_CHUNK 1024  /* ratings of one chunk of anirec_fold_in_split: part of its definition, not a knob */

enum {
  ANIREC_OK = 0,
  ANIREC_EINVAL = -1,     /* bad argument (null pointer, size out of range, dim not one of 32, 64, 128, 256) */
  ANIREC_ENODEVICE = -2,  /* no HIP device / wrong architecture */
  ANIREC_EWORKSPACE = -3, /* workspace too small */
  ANIREC_ECAPTURE = -4,   /* graph capture / instantiate failed */
  ANIREC_ECOMM = -5       /* an RCCL call failed */
};

int anirec_abi_version(void);
/* Human-readable text for a status code returned by this library. */
const char *anirec_status_string(int status);
/* Name of the device the library would run on; returns status. */
int anirec_device_name(char *buf_host, size_t buf_len);

/* ------------------------------------------------------------------------- *
 *  TRAINING  — replaces model.fit's train step, neural_network/neural_network.py:210-217
 *  (graph built at :66-106: Embedding x2 -> Dot(normalize) -> Dense(1) -> BatchNorm
 *   -> sigmoid; binary_crossentropy + whole-table L2; Keras-2.12 Adam, dense update).
 * ------------------------------------------------------------------------- */

/* Update rule of the dense optimiser step (anirec_train_desc::optimizer): the Keras-2.12 optimisers with their
 * default hyper-parameters that model.compile(optimizer=...) resolves by name (neural_network.py:102-104).  fp32,
 * never contracted into FMA, g = chunk sums + 2*l2*W, lr = float32(lrfn(epoch)):
 *   ADAM     m += (g-m)*0.1; v += (g*g-v)*0.001; w -= (m*alpha)/(sqrt(v)+1e-7)   slots m, v (init 0)
 *   SGD      w -= g*lr                                                             (momentum 0; no slot)
 *   RMSPROP  v = 0.9*v + 0.1*(g*g); w -= (lr*g)*(1/sqrt(v+1e-7))                  (rho 0.9, not centred; init 0)
 *   ADAGRAD  v = v + g*g; w -= (lr*g)/sqrt(v+1e-7)                                  (accumulator, init 0.1)
 * The one slot of RMSprop / Adagrad lives in V (and anirec_state.adam_v for the four head scalars); M and
 * anirec_state.adam_m are not touched by them.  sqrt and divide are correctly rounded. */
enum {
  ANIREC_OPT_ADAM = 0,
  ANIREC_OPT_SGD = 1,
  ANIREC_OPT_RMSPROP = 2,
  ANIREC_OPT_ADAGRAD = 3
};

/* Output head of the model (anirec_train_desc::loss / ::activation; the predict entry points' `activation`): Keras 2.12's
 * losses and output activations that model.compile(loss=...) and Activation(...) resolve by name (neural_network.py:
 * 97-104).  y = BatchNorm output, p = act(y), t = scaled rating, e = p - t, B = global batch; the data loss is
 * sum_i l(p_i, t_i) / B and dy_i = l'(p_i, t_i) * act'(y_i) / B (Keras SUM_OVER_BATCH_SIZE).
 *   ACT_SIGMOID   sigmoid(y)                            act' = p(1-p)
 *   ACT_LINEAR    y                                     1
 *   ACT_TANH      tanh(y)                               1 - p^2
 *   ACT_RELU      max(y, 0)                             y > 0 ? 1 : 0
 *   ACT_SOFTPLUS  max(y,0) + log1p(exp(-|y|))           sigmoid(y)
 *   LOSS_BCE      with ACT_SIGMOID: from logits, max(y,0) - y t + log1p(exp(-|y|)), dy = (p - t)/B;
 *                 else q = clip(p, 1e-7, 1-1e-7): -(t log(q+1e-7) + (1-t) log(1-q+1e-7)), gradient through q
 *                 (0 outside the closed clip interval)
 *   LOSS_MSE      e^2                                   2e
 *   LOSS_MAE      |e|                                   sign(e), 0 at 0
 *   LOSS_HUBER    |e| <= 1 ? e^2/2 : |e| - 1/2          |e| <= 1 ? e : sign(e)
 *   LOSS_LOGCOSH  e + softplus(-2e) - log 2             1 - 2 sigmoid(-2e)
 * Every activation is non-decreasing: the top-k paths rank by the cosine and re-score through the head.  0, 0 is the
 * reference's default model (sigmoid + binary_crossentropy). */
enum {
  ANIREC_LOSS_BCE = 0,
  ANIREC_LOSS_MSE = 1,
  ANIREC_LOSS_MAE = 2,
  ANIREC_LOSS_HUBER = 3,
  ANIREC_LOSS_LOGCOSH = 4
};
enum {
  ANIREC_ACT_SIGMOID = 0,
  ANIREC_ACT_LINEAR = 1,
  ANIREC_ACT_TANH = 2,
  ANIREC_ACT_RELU = 3,
  ANIREC_ACT_SOFTPLUS = 4
};

/* One optimiser step of the schedule.  `alpha` is Adam's bias-corrected step size
 * lr*sqrt(1-b2^t)/(1-b1^t) for this step, or `lr` for the other kinds, computed on the host from lrfn(epoch)
 * (neural_network.py:109-125) so host and oracle agree bit-for-bit. */
typedef struct anirec_step {
  int32_t start; /* first rating of this rank's part of the batch in the epoch arrays */
  int32_t count; /* ratings of this rank in the batch (<= max_batch) */
  float alpha;
  int32_t global_count; /* ratings of the batch over all ranks (== count on one GPU) */
} anirec_step;

/* Device-resident scalar state; one instance per model.  Layout is ABI. */
typedef struct anirec_state {
  /* trainable scalars: Dense(1) kernel/bias (neural_network.py:97), BN gamma/beta (:99) */
  float w, b, gamma, beta;
  float adam_m[4], adam_v[4]; /* Adam slots of the four scalars, same order */
  float mov_mean, mov_var;    /* BatchNormalization moving statistics */
  float reg_sumsq;            /* sum(U_local^2)+sum(A^2) of the tables this step read (L2 term / lambda) */
  float bn_mu, bn_var;        /* batch statistics of the last training step */
  float last_loss, last_mse;  /* total loss (incl. L2) and mse of the last training step */
  int32_t step_fwd;           /* schedule cursor of the next fwd+head */
  int32_t step_bwd;           /* schedule cursor of the next bwd+adam */
  int32_t pad0;
  /* epoch accumulators (Keras History semantics: sample-weighted means) */
  double loss_wsum;   /* sum over steps of count*total_loss */
  double se_sum;      /* sum of squared errors (mse numerator) */
  double n_seen;      /* ratings seen */
  /* validation accumulators, BN inference mode (neural_network.py:216) */
  double val_bce_sum; /* sum of per-row data loss (BCE by default; the descriptor's loss) */
  double val_se_sum;
  double val_n;
  /* the same epoch loss split for user-partitioned multi-GPU runs: the caller adds the
   * other ranks' user-table terms.  sums over steps of count * {bce, sum(U_local^2), sum(A^2)}; bce = the data term of
   * the descriptor's loss */
  double bce_wsum, reg_user_wsum, reg_anime_wsum;
  float reg_user_sumsq, reg_anime_sumsq; /* split of reg_sumsq */
} anirec_state;

typedef struct anirec_train_desc {
  int32_t n_user_rows;  /* user rows held by this rank */
  int32_t n_anime_rows; /* anime rows (replicated) */
  int32_t max_batch;    /* capacity of per-step buffers, 1..ANIREC_MAX_BATCH */
  int32_t arena_steps;  /* number of steps the prep arena holds */
  int32_t dense_mode;   /* 0: one GPU, gradients stay chunked.
                           1: user-sharded data parallelism — bwd also writes the ANIME rows' gradient into
                              `dense_grad`, the caller all-reduces it (RCCL), adam reads it;
                           2: replicated tables (the reference's TPUStrategy shape, neural_network.py:173-178)
                              — EVERY row's gradient goes through `dense_grad` (all-reduce, or reduce-scatter
                              with adam_row_lo/hi = this rank's row shard) */
  int32_t n_seg;        /* head packets to read: 1 on one GPU, world size when all-gathered */
  int32_t my_seg;       /* this rank's packet */
  int32_t dense_rows;   /* rows of dense_grad: >= the rows it carries (n_anime_rows in mode 1, all rows in
                           mode 2); extra rows are zero padding up to a multiple of the world size */
  float l2;             /* lambda of embeddings_regularizer L2 (neural_network.py:73) */
  int32_t adam_row_lo;  /* mode 2: adam updates table rows [adam_row_lo, adam_row_hi) only (the caller */
  int32_t adam_row_hi;  /* all-gathers W afterwards); 0,0 = every row */
  int32_t lazy;         /* != 0 (`lazy_state` set): the dense update of the rows a batch does not touch is deferred —
                           dense_mode 0: both tables, inside anirec_trainer_run; dense_mode 1: the rank's user rows,
                           inside anirec_dist_run / the stepper calls (LAZY USER ROWS); ignored in dense_mode 2 */
  /* tables: rows [0,n_user_rows) users, then n_anime_rows anime; [rows][128] fp32 ([rows][dim] for the _w calls).
   * W = embeddings, M/V = Adam first/second moments. */
  float *W, *M, *V;
  int32_t *rowmap;      /* [2][n_user_rows+n_anime_rows] (one map per step parity); zero before first use, left zero */
  anirec_state *state;
  /* this rank's ratings in epoch (shuffled) order; user_idx are LOCAL user rows */
  const int32_t *user_idx;
  const int32_t *anime_idx;
  const float *rating;
  const anirec_step *sched; /* [n_steps] */
  int32_t n_steps;
  int32_t loss;         /* ANIREC_LOSS_*: the data loss of the head stage and of anirec_eval (0 = binary_crossentropy) */
  /* head packets: n_seg packets of anirec_packet_floats(max_batch) floats each; packet
   * my_seg is written by the fwd kernel, the others by the caller's all-gather. */
  float *packets;
  float *dense_grad;    /* [dense_rows*128] gradients then [dense_rows] self-coefficient sums, or NULL (128 only) */
  void *workspace;      /* >= anirec_train_workspace_bytes(max_batch, arena_steps) (_w calls: ..._bytes_w(max_batch,
                           arena_steps, dim)); zero before first use */
  size_t workspace_bytes;
  void *lazy_state;     /* lazy != 0: anirec_train_lazy_bytes(rows) bytes, zero before first use; else NULL */
  int32_t optimizer;    /* ANIREC_OPT_*: the update rule of the adam stage.  The lazy update exists for ADAM only: a
                           descriptor with lazy != 0 and another kind is rejected (ANIREC_EINVAL) by every call */
  int32_t activation;   /* ANIREC_ACT_*: the output activation (0 = sigmoid).  loss / activation out of range: every call
                           that takes the descriptor returns ANIREC_EINVAL before it enqueues anything */
} anirec_train_desc;
/* A descriptor must be zero-initialised before its fields are set: fields added in the struct's former padding (loss,
 * activation) then read 0, the reference's default model. */

/* floats in one head packet: c[pcap], t[pcap], 4 ints {count,0,0,0}; pcap = max_batch rounded
 * up to a multiple of 4 */
size_t anirec_packet_floats(int32_t max_batch);
size_t anirec_train_workspace_bytes(int32_t max_batch, int32_t arena_steps);
/* the workspace holds the chunk partial rows, so its size and its layout depend on the width: every call that takes
 * the descriptor's workspace has a _w twin */
size_t anirec_train_workspace_bytes_w(int32_t max_batch, int32_t arena_steps, int32_t dim);
/* per-row state of the lazy dense Adam: the step each row has been updated to + its sum(W^2) of the window's steps */
size_t anirec_train_lazy_bytes(int32_t table_rows);

/* state.reg_sumsq <- sum(W^2) (both tables).  Call once after (re)loading weights. */
int anirec_train_init_reg(const anirec_train_desc *d, void *stream);
int anirec_train_init_reg_w(const anirec_train_desc *d, int32_t dim, void *stream);

/* Sort each batch of steps [first_step, first_step+n_steps) by table row and cut the
 * per-row runs into chunks (<= ANIREC_CHUNK ratings) for the backward pass.  Results
 * land in arena slot (step % arena_steps).  Replaces TF's IndexedSlices ->
 * unsorted_segment_sum densification inside model.fit. */
int anirec_train_prep(const anirec_train_desc *d, int32_t first_step, int32_t n_steps, void *stream);
int anirec_train_prep_w(const anirec_train_desc *d, int32_t dim, int32_t first_step, int32_t n_steps, void *stream);

/* The four stages of one step.  They read the step index from device memory (state->step_fwd /
 * state->step_bwd / a workspace word head publishes) so that a captured graph can be replayed for every step;
 * the per-step scratch is double-buffered by step parity:
 *   fwd  : gather U[ui], A[ai]; c = <l2n(u), l2n(a)>      -> packet, su, sa
 *   head : Dense(1) + BatchNorm(batch stats over ALL packets) + the activation and loss of the descriptor,
 *          d loss / d y per rating and the batch partial sums
 *   bwd  : closed-form backward to d loss / d c, per-chunk weighted row sums of the OTHER
 *          table -> chunk partials (+rowmap)
 *   adam : dense fused Adam over every row of both tables, g = sparse + 2*l2*W, emits
 *          sum(W_new^2) partials; then Adam on the 4 scalars, moving stats, epoch
 *          metrics, step_fwd++                                                           */
int anirec_train_fwd(const anirec_train_desc *d, void *stream);
int anirec_train_head(const anirec_train_desc *d, void *stream);
int anirec_train_bwd(const anirec_train_desc *d, void *stream);
int anirec_train_adam(const anirec_train_desc *d, void *stream);
/* The stages at width dim (tables, workspace and dense one-GPU descriptor of that width).  prep and head do
 * width-independent work (a sort of indices; one dot product per rating) but find their arrays in the workspace, whose
 * layout depends on the width. */
int anirec_train_fwd_w(const anirec_train_desc *d, int32_t dim, void *stream);
int anirec_train_head_w(const anirec_train_desc *d, int32_t dim, void *stream);
int anirec_train_bwd_w(const anirec_train_desc *d, int32_t dim, void *stream);
int anirec_train_adam_w(const anirec_train_desc *d, int32_t dim, void *stream);
/* Measurement hook (bench.py): while armed, the training kernels stamp each workgroup's first / last instruction
 * with the 100 MHz constant clock and every launch is followed by a synchronisation that turns the stamps into one
 * duration.  Returns per kernel — 0 fwd, 1 head, 2 bwd, 3 adam, 4 lazy catch-up, 5 lazy adam, 6 lazy flush, 7 lazy
 * reduce — the mean duration [us] of the launches since the last call (-1 = none) and their count (either pointer
 * may be NULL), then arms (enable != 0) or disarms.  Armed steps never replay the captured graph. */
int anirec_train_stage_ticks(const anirec_train_desc *d, int32_t enable, float *us8_host, int32_t *launches8_host,
                             void *stream);

/* adam as two launches (dense_mode 1): which == 1 updates the user rows (may run while the anime gradient is
 * still in the all-reduce), which == 2 the anime rows and finishes the step.  ANIREC_EINVAL with lazy user rows
 * (below), before anything is launched: their update is only kept by the stepper's run and block protocol. */
int anirec_train_adam_part(const anirec_train_desc *d, int32_t which, void *stream);

/* Multi-GPU step as three C calls and two collectives (dense_mode 1 or 2; the stepper owns a side stream):
 *     anirec_train_fwd                      -> all-gather of the head packets (BatchNorm sees the global batch)
 *     anirec_dist_step_mid  (head, bwd, densify; mode 1 forks the user-row adam onto the side stream)
 *                                           -> all-reduce / reduce-scatter of dense_grad
 *     anirec_dist_step_back (joins the side stream; adam of the rows that needed the collective; step finish)
 *   [mode 2 with a row shard: all-gather of W] */
typedef struct anirec_dist_stepper anirec_dist_stepper;
int anirec_dist_stepper_create(const anirec_train_desc *d, anirec_dist_stepper **out_host);
int anirec_dist_stepper_destroy(anirec_dist_stepper *h);
/* anirec_dist_step_front = anirec_train_fwd, preceded — lazy user rows, below — by the catch-up of the batch's rows
 * when the step is the first of its prepared block. */
int anirec_dist_step_front(anirec_dist_stepper *h, void *stream);
int anirec_dist_step_mid(anirec_dist_stepper *h, void *stream);
int anirec_dist_step_back(anirec_dist_stepper *h, void *stream);
/* LAZY USER ROWS (desc->lazy != 0 with dense_mode 1; see LAZY DENSE ADAM below).  In the user-sharded step the dense
 * Adam stream over the rank's user rows becomes: sparse step of the rows the batch touched (forked beside densify +
 * all-reduce; the catch-up of the next batch's rows rides partly in the head launch, partly in that forked launch), a
 * flush of the user rows every ANIREC_LAZY_WINDOW steps and at the end of a run.  The replicated anime rows keep their dense update behind the all-reduce.  Tables, Adam moments
 * and scalar state stay bit-identical to the dense step; reg_user_wsum / loss_wsum receive the user rows' L2 term at
 * the flush.  A caller that drives the steps itself must tell the stepper where it is: _begin(first_step, n_steps)
 * once per run (the tables are current there; stream-ordered) and _block(n) after every anirec_train_prep of n steps;
 * without them the step calls of a lazy descriptor return ANIREC_EINVAL.  anirec_dist_run does both itself. */
int anirec_dist_stepper_begin(anirec_dist_stepper *h, int32_t first_step, int32_t n_steps, void *stream);
int anirec_dist_stepper_block(anirec_dist_stepper *h, int32_t n_steps);

/* The same loop inside the library, the collectives issued to RCCL from C on the engine's stream (one call per
 * block of steps instead of three C calls and two torch.distributed calls per step).  Replaces the reference's only
 * data-parallel construct, neural_network/neural_network.py:142-147,173-178 (replicated variables under a strategy
 * scope: a dense gradient all-reduce per step).  RCCL is bound at run time: anirec_rccl_load(NULL) takes the copy the
 * process has mapped already (torch's) or loads librccl.so.1; ANIREC_ENODEVICE if there is none.
 *   rank 0: anirec_rccl_unique_id(id) -> the caller broadcasts the ANIREC_RCCL_ID_BYTES bytes -> every rank:
 *   anirec_dist_comm_create(id, rank, world) (collective; the current HIP device) -> anirec_dist_run(...) per epoch. */
#define ANIREC_RCCL_ID_BYTES 128
int anirec_rccl_load(const char *path_host);
int anirec_rccl_unique_id(char *id_host);
typedef struct anirec_dist_comm anirec_dist_comm;
int anirec_dist_comm_create(const char *id_host, int32_t rank, int32_t world, anirec_dist_comm **out_host);
int anirec_dist_comm_destroy(anirec_dist_comm *c);
/* steps [first_step, first_step + n_steps) of the stepper's descriptor (n_seg = world, my_seg = rank); the packet
 * all-gather, the gradient all-reduce / reduce-scatter and the W all-gather run in place on the descriptor's buffers.
 * first_step must equal the device cursor.  use_graph != 0: blocks of min(32, arena_steps/2) steps, collectives
 * included, are captured once and replayed (every rank must pass the same value); a failed capture falls back to
 * eager launches. */
int anirec_dist_run(anirec_dist_stepper *h, anirec_dist_comm *c, int32_t first_step, int32_t n_steps, int32_t use_graph,
                    void *stream);

/* LAZY DENSE ADAM (desc->lazy).  Keras' Adam updates every row of both tables every step, because the L2 regulariser
 * gives every row a gradient (2 lambda W) — 28 B/element/step of HBM traffic for rows the batch never touched.  Each
 * element's update sequence is independent of every other element's, so the rows a batch does not touch can take
 * their pure-L2 steps LATER, several at a time, in registers, with the same fp32 operations in the same order:
 *   catch-up(t)  brings the rows batch t touches up to step t (their pending L2-only steps), before fwd(t) reads them
 *                (extra workgroups of step t-1's head and sparse-adam launches; fwd(t-1) marks which rows batch t-1
 *                itself will bring up to date);
 *   sparse adam(t) applies step t (chunk gradient + 2 lambda W) to those rows only;
 *   every ANIREC_LAZY_WINDOW steps (and at the end of every anirec_trainer_run call) a flush replays the pending
 *   steps of every row — one streaming pass over W, M, V per window instead of one per step — and a reduce kernel
 *   assembles the per-step sum(W^2) of the loss's L2 term from the per-row values the replays recorded.
 * Tables, Adam moments and the scalar state are BIT-IDENTICAL to the dense path; the History loss agrees to fp32
 * rounding of its L2 sum (another summation order).  Outside anirec_trainer_run the tables are always up to date. */

/* Steps [first_step, first_step + n_steps) — prep, fwd, head, bwd, adam — on one GPU; first_step
 * must equal the device cursor state->step_fwd.  use_graph != 0 replays a captured hipGraph of
 * G = min(32, arena_steps/2) steps whose first node prepares the G steps after it, so no host
 * work is needed between replays. */
typedef struct anirec_trainer anirec_trainer; /* host-side handle: descriptor copy + graph cache */
int anirec_trainer_create(const anirec_train_desc *d, anirec_trainer **out_host);
/* a handle for tables of width dim; it carries the width: _run, _set_metrics and _destroy are the same calls */
int anirec_trainer_create_w(const anirec_train_desc *d, int32_t dim, anirec_trainer **out_host);
int anirec_trainer_destroy(anirec_trainer *t);
int anirec_trainer_run(anirec_trainer *t, int32_t first_step, int32_t n_steps, int32_t use_graph,
                       void *stream);

/* Validation pass on n rows (BN inference, moving stats): accumulates
 * state->val_* ; val_loss = val_bce_sum/val_n + l2*reg_sumsq  (neural_network.py:216).  val_bce_sum and the state's
 * bce_wsum carry the data term of the descriptor's loss (the name is historical). */
int anirec_eval(const anirec_train_desc *d, const int32_t *user_idx, const int32_t *anime_idx,
                const float *rating, int32_t n, void *stream);

/* Keras metrics of model.compile(metrics=...) (neural_network.py:102-104), accumulated on the GPU beside the train
 * step and the validation pass.  Per rating, e = p - t, p = the head's output:
 *   MAE      |e|                                     MAPE  100 |e| / max(|t|, 1e-7)
 *   MSLE     (log(max(p, 1e-7) + 1) - log(max(t, 1e-7) + 1))^2
 *   LOGCOSH  the LOSS_LOGCOSH term                   BCE   the LOSS_BCE term of the descriptor's activation
 *   ACC      1 if t == (p > 0.5) else 0 (binary_accuracy)
 *   AUC      Keras AUC() with its 200 evenly spaced thresholds: bucket max(ceil(p * 199) - 1, 0) (fp32 product)
 *            receives the fixed-point label mass wt = rint(clamp(t, 0, 1) * 2^20) as positive and 2^20 - wt as
 *            negative mass (integer sums: bitwise reproducible); the caller forms TP / FP as reverse cumulative sums
 *            and the ROC area by the trapezoidal rule.  Sigmoid heads only (Keras asserts p in [0, 1]).
 * MSE and RootMeanSquaredError come from state->se_sum / val_se_sum and need no bit.  Epoch values are the sums
 * divided by state->n_seen (train) or val_n (validation). */
enum {
  ANIREC_METRIC_MAE = 1,
  ANIREC_METRIC_MAPE = 2,
  ANIREC_METRIC_MSLE = 4,
  ANIREC_METRIC_LOGCOSH = 8,
  ANIREC_METRIC_BCE = 16,
  ANIREC_METRIC_ACC = 32,
  ANIREC_METRIC_AUC = 64
};
#define ANIREC_METRIC_KINDS 6   /* the scalar kinds: bits 0..5, the order of anirec_metric_acc.sum */
#define ANIREC_AUC_BINS 200     /* AUC thresholds */
#define ANIREC_AUC_ONE (1u << 20) /* label mass of one rating in the AUC bins */
typedef struct anirec_metric_acc { /* device-resident; zeroed by the caller at epoch / validation start */
  double sum[ANIREC_METRIC_KINDS];  /* MAE, MAPE, MSLE, LOGCOSH, BCE, ACC: sums of the per-rating values */
  uint64_t auc_pos[ANIREC_AUC_BINS], auc_neg[ANIREC_AUC_BINS]; /* label mass per bucket, units of 2^-20 */
} anirec_metric_acc;
/* The metric set of a handle's runs (anirec_trainer_run / anirec_dist_run and the stepper's step calls): every step
 * adds the requested kinds of the whole (global) batch to *acc — on every rank, no collective needed.  Mask 0 or a
 * NULL acc: no metrics, the step as without this call.  Bits outside ANIREC_METRIC_* or AUC with an activation other
 * than ANIREC_ACT_SIGMOID: ANIREC_EINVAL, the handle unchanged.  Drops the handle's captured graph.  The stage calls
 * (anirec_train_head, ...) never accumulate metrics. */
int anirec_trainer_set_metrics(anirec_trainer *t, uint32_t mask, anirec_metric_acc *acc);
int anirec_dist_stepper_set_metrics(anirec_dist_stepper *h, uint32_t mask, anirec_metric_acc *acc);
/* anirec_eval that also adds the requested kinds of the n validation rows to *acc (same checks as above). */
int anirec_eval_metrics(const anirec_train_desc *d, uint32_t mask, anirec_metric_acc *acc, const int32_t *user_idx,
                        const int32_t *anime_idx, const float *rating, int32_t n, void *stream);
/* at width dim; mask 0 with a NULL acc is anirec_eval at that width */
int anirec_eval_metrics_w(const anirec_train_desc *d, int32_t dim, uint32_t mask, anirec_metric_acc *acc,
                          const int32_t *user_idx, const int32_t *anime_idx, const float *rating, int32_t n,
                          void *stream);

/* Standalone fused Adam on a flat fp32 array with an explicit dense gradient
 * (Keras-2.12 Adam dense branch; bit-exact to the oracle given the same g). */
int anirec_adam_flat(float *w, float *m, float *v, const float *g, size_t n, float alpha,
                     void *stream);
/* The same for the one-slot kinds (ANIREC_OPT_SGD / _RMSPROP / _ADAGRAD; the header's formulas, bit-exact given the
 * same g): `slot` is the RMSprop / Adagrad slot (ignored by SGD, may be NULL there), `rate` is lr.  ADAM has two
 * slots: ANIREC_EINVAL, use anirec_adam_flat. */
int anirec_opt_flat(int32_t kind, float *w, float *slot, const float *g, size_t n, float rate, void *stream);

/* Self-test of the lazy update's short arithmetic sequences (tests only; no reference call site — it guards the claim
 * that the lazy dense Adam performs the dense kernel's fp32 operations): the correctly rounded square root the replay
 * uses is compared with sqrtf on EVERY float of [2^-96, 2^96], its divide with IEEE `/` on n_div pseudo-random operand
 * pairs of the admitted ranges.  counts2[0] / counts2[1] (device, uint64) receive the numbers of mismatches. */
int anirec_selftest_lazy_math(uint64_t n_div, uint64_t *counts2, void *stream);

/* Self-test of the replay's one-correction divide (tests only).  mode 0: its refined reciprocal against 1.0f / d on
 * EVERY float whose bits lie in [lo, hi]; mode 1: the quotient against IEEE `/` on every significand pair n, d in
 * [1, 2) with d's 23 significand bits in [lo, hi) (hi <= 2^23) and all 2^23 n's; mode 2: the same for the uncorrected
 * product n * y (must report misses).  counts4 (device, uint64): mismatches, operands checked, min / max bits of a
 * failing d (~0 / 0 if none). */
int anirec_selftest_lazy_div(int32_t mode, uint32_t lo, uint32_t hi, uint64_t *counts4, void *stream);

/* Self-test of the lazy replay on given rows (tests only): wmv = W, M, V planes [3][rows][128] (device fp32); every
 * row takes the L2-only Adam steps [j0[row], nj) of alpha8[0..nj) (nj <= ANIREC_LAZY_WINDOW) once by the replay
 * (short sequences, range test, redo by the full expansions) into out_lazy, once by the dense update into out_dense
 * (same layout); fast[row] = 1 if the row passed the short sequences' range test — the flush's once-per-row test
 * (row_test != 0) or the catch-up's per-step one. */
int anirec_selftest_lazy_replay(const float *wmv, int32_t rows, const float *alpha8, int32_t nj, const int32_t *j0,
                                float two_l2, int32_t row_test, float *out_lazy, float *out_dense, int32_t *fast,
                                void *stream);

/* Epoch shuffle: out[i] = in[perm[i]] for the three rating columns (model.fit shuffle=True). */
int anirec_gather_ratings(const int32_t *user_in, const int32_t *anime_in, const float *rating_in,
                          const int64_t *perm, size_t n, int32_t *user_out, int32_t *anime_out,
                          float *rating_out, void *stream);

/* ------------------------------------------------------------------------- *
 *  SIMILARITY — replaces get_weights + np.dot + np.argsort,
 *  similar_anime/similar_anime.py:136-171,404-408 ; similar_users/similar_users.py:75-101,293-296
 * ------------------------------------------------------------------------- */

/* What = W / ||W||_2 row-wise, no epsilon (zero row -> NaN like NumPy). */
int anirec_rownorm(const float *W, int32_t n, float *What, void *stream);
int anirec_rownorm_w(const float *W, int32_t n, int32_t dim, float *What, void *stream);

/* scores[j] = <What[j], What[q]> for every row j (k-ordered fp32 fma chain).  _w: the same chain over
 * k = 0 .. dim-1 in index order. */
int anirec_cosine_scores(const float *What, int32_t n, int32_t q, float *scores, void *stream);
int anirec_cosine_scores_w(const float *What, int32_t n, int32_t dim, int32_t q, float *scores, void *stream);

/* Top-k rows by descending score for a batch of query rows of the same table.
 *   queries[nq]   : query row indices
 *   keep[n]       : optional byte mask (1 = candidate allowed), NULL = all
 *   exclude_self  : drop the query row itself (similar_users.py:303, similar_anime.py:459)
 *   out_idx[nq*k] : row indices (-1 padded), out_score[nq*k] : fp32 scores (NaN padded)
 * Ties: ascending row index.  NaN scores rank last.  k <= ANIREC_MAX_TOPK.
 * workspace: anirec_topk_workspace_bytes(n, nq) bytes. */
size_t anirec_topk_workspace_bytes(int32_t n, int32_t nq);
int anirec_cosine_topk(const float *What, int32_t n, const int32_t *queries, int32_t nq,
                       const uint8_t *keep, int32_t exclude_self, int32_t k, int32_t *out_idx,
                       float *out_score, void *workspace, size_t workspace_bytes, void *stream);
/* (the workspace holds score rows only: anirec_topk_workspace_bytes serves every width) */
int anirec_cosine_topk_w(const float *What, int32_t n, int32_t dim, const int32_t *queries, int32_t nq,
                         const uint8_t *keep, int32_t exclude_self, int32_t k, int32_t *out_idx,
                         float *out_score, void *workspace, size_t workspace_bytes, void *stream);

/* anirec_cosine_topk for ANY k >= 1 (a whole ranking included): the same scores, candidates, order, ties and
 * padding, and for k <= ANIREC_MAX_TOPK the same output.  The radix select finds the k-th key, the winners are
 * collected per query and sorted in LDS (k <= 20480) or as LDS tiles plus merge passes (larger k).
 * workspace: anirec_topk_large_workspace_bytes(n, nq, k) bytes (it grows with min(k, n)); less, down to one
 * query's share, runs the queries in smaller batches. */
size_t anirec_topk_large_workspace_bytes(int32_t n, int32_t nq, int32_t k);
int anirec_cosine_topk_large(const float *What, int32_t n, const int32_t *queries, int32_t nq,
                             const uint8_t *keep, int32_t exclude_self, int32_t k, int32_t *out_idx,
                             float *out_score, void *workspace, size_t workspace_bytes, void *stream);
/* (anirec_topk_large_workspace_bytes serves every width) */
int anirec_cosine_topk_large_w(const float *What, int32_t n, int32_t dim, const int32_t *queries, int32_t nq,
                               const uint8_t *keep, int32_t exclude_self, int32_t k, int32_t *out_idx,
                               float *out_score, void *workspace, size_t workspace_bytes, void *stream);

/* Same result as anirec_cosine_topk on the matrix cores: fp16 MFMA candidate scores for all
 * keys with a rigorous error window, exact fp32 fma-chain re-rank of the survivors.
 * The error window is proven for UNIT-NORM rows (the output of anirec_rownorm, as every reference call
 * site passes: similar_users.py:293 takes get_weights() output).  The conversion pass checks it: if any
 * finite key or query row has | ||row||^2 - 1 | > 1e-3 every query is flagged (flags bit 2) and falls to the
 * caller's exact re-run, so un-normalised input is slow, never silently incomplete.
 * flags[nq] (device) is non-zero for the rare query whose window could not be proven
 * complete (dense ties / more than 256 survivors); its output row is -1/NaN and the caller
 * re-runs it through anirec_cosine_topk.  k <= ANIREC_MAX_TOPK - 1.
 * A PRIOR theta0 for every row's threshold (prior_mode 1 and 2 below; otherwise -4, below every cosine) means a
 * candidate must score >= max(theta0, what the keys seen so far prove).  A good guess of the rows' final k-th best
 * score (minus a margin) spares most of the ~k ln(n) early appends per row.  Results stay exact: a row whose true
 * threshold lies below theta0 ends with too few candidates, is flagged like any other unproven row, and the caller
 * re-runs it (without a prior, or through anirec_cosine_topk).
 * The whole similar_anime / similar_users job (every row a query: similar_users.py:290-312 at BASELINE configs[3]
 * scale) is ONE call: the keys are converted once, the queries run in batches [starts[b], starts[b+1]), and the
 * batches are dealt to `lanes` stream-ordered chains (the caller's stream + side streams the library keeps, forked and
 * joined by events inside this call; 1 <= lanes <= 4) so that one batch's per-row refresh / re-rank waves run beside
 * another batch's MFMA kernel.  prior_mode 0: no prior; 1: the first `learn_batches` (0 or 1) batches run alone and
 * the k-th best scores of their rows give the others a prior, computed on the device (no host round trip); 2: theta0
 * (-4 <= theta0 <= 1).
 * flags[nq] as above: the caller re-runs flagged rows (without a prior, then through
 * anirec_cosine_topk).  Results are identical to anirec_cosine_topk whatever the plan.
 * prior_mode 3 = mode 1 for the ALL-PAIRS job (queries[i] == i for all i < nq == n, keep == NULL; checked on the
 * device: any other query list flags every row): cosine(i, j) == cosine(j, i), so a batch computes the dot products of
 * its rows with the rows of LATER batches once, for both — a score that reaches the learnt prior is also dropped into
 * the later row's inbox (through per-wave logs a side kernel deals out) — and skips the key tiles of EARLIER batches
 * (their pairs are in its inboxes already): ~0.65 of the MFMA work at 350 k rows.  An inbox that overflows flags its row
 * like any unproven row.  Needs the learning batch, whole 128-row key tiles per batch (the default plan has them) and lanes <= 2;
 * otherwise the call runs as mode 1.  Results are identical either way.  Workspace:
 * anirec_cosine_topk_allpairs_workspace_bytes (the job's + two inboxes of n x 256 entries + the chains' logs).
 * anirec_cosine_topk_job_plan fills the library's default plan: starts_host[ANIREC_TOPK_MAX_BATCHES + 1];
 * max_batch <= 0 and lanes <= 0 select the defaults (131072 rows, 2 lanes).
 * workspace: anirec_cosine_topk_job_workspace_bytes(n, rows of the largest batch, lanes). */
int anirec_cosine_topk_job_plan(int32_t nq, int32_t k, int32_t prior_auto, int32_t max_batch, int32_t lanes,
                                int32_t *starts_host, int32_t *n_batches_host, int32_t *learn_batches_host);
size_t anirec_cosine_topk_job_workspace_bytes(int32_t n, int32_t max_batch_rows, int32_t lanes);
size_t anirec_cosine_topk_allpairs_workspace_bytes(int32_t n, int32_t max_batch_rows, int32_t lanes);
/* the all-pairs plan: the learning batch + `main_batches` (<= 0: 2 round(n / 88 000), clamped to 2..8) batches of equal
 * WORK (a later batch streams fewer keys and takes more rows); the default plan when the job is too small to learn */
int anirec_cosine_topk_allpairs_plan(int32_t n, int32_t k, int32_t lanes, int32_t main_batches, int32_t *starts_host,
                                     int32_t *n_batches_host, int32_t *learn_batches_host);
int anirec_cosine_topk_job(const float *What, int32_t n, const int32_t *queries, int32_t nq, const uint8_t *keep,
                           int32_t exclude_self, int32_t k, int32_t prior_mode, float theta0,
                           const int32_t *starts_host, int32_t n_batches, int32_t learn_batches, int32_t lanes,
                           int32_t *out_idx, float *out_score, int32_t *flags, void *workspace,
                           size_t workspace_bytes, void *stream);

/* Measurement hook (bench.py's roofline leg): returns the summed HIP-event duration [ms] and the number of the
 * MFMA candidate-kernel launches of the calls made since it was last armed, then arms (enable != 0) or disarms
 * the timing.  Armed calls block until the stream drains, and an armed job runs its batches on ONE chain so that
 * every timed launch runs alone. */
int anirec_topk_mfma_timing(int32_t enable, float *cand_ms, int32_t *launches);

/* ------------------------------------------------------------------------- *
 *  PREDICTION — replaces model.predict([user_arr, anime_arr]), model_recs/model_recs.py:394
 * ------------------------------------------------------------------------- */

/* Inference head: act(gamma*(w*c+b-mov_mean)/sqrt(mov_var+1e-3)+beta); the five entry points below without an
 * `activation` argument use ANIREC_ACT_SIGMOID, each *_act variant takes ANIREC_ACT_* (ANIREC_EINVAL out of range,
 * before anything is enqueued). */
typedef struct anirec_head {
  float w, b, gamma, beta, mov_mean, mov_var;
} anirec_head;

/* p[i] = model(user_idx[i], anime_idx[i]) for n explicit pairs. */
int anirec_predict_pairs(const float *U, const float *A, const int32_t *user_idx,
                         const int32_t *anime_idx, int32_t n, const anirec_head *head_host,
                         float *p, void *stream);

int anirec_predict_pairs_act(const float *U, const float *A, const int32_t *user_idx,
                             const int32_t *anime_idx, int32_t n, const anirec_head *head_host,
                             int32_t activation, float *p, void *stream);
int anirec_predict_pairs_w(const float *U, const float *A, int32_t dim, const int32_t *user_idx,
                           const int32_t *anime_idx, int32_t n, const anirec_head *head_host,
                           int32_t activation, float *p, void *stream);

/* Workspace of predict_grid / predict_topk: l2-normalised copies of A and of the query
 * users (+ a batch of rating rows when topk != 0). */
size_t anirec_predict_workspace_bytes(int32_t n_anime, int32_t n_users, int32_t topk);
size_t anirec_predict_workspace_bytes_w(int32_t n_anime, int32_t n_users, int32_t topk, int32_t dim);

/* out[j*n_anime + a] = model(users[j], a) for every anime a (the full rating grid). */
int anirec_predict_grid(const float *U, const float *A, int32_t n_anime, const int32_t *users,
                        int32_t n_users, const anirec_head *head_host, float *out,
                        void *workspace, size_t workspace_bytes, void *stream);
int anirec_predict_grid_act(const float *U, const float *A, int32_t n_anime, const int32_t *users,
                            int32_t n_users, const anirec_head *head_host, int32_t activation, float *out,
                            void *workspace, size_t workspace_bytes, void *stream);
/* the _w predict calls take the activation (as the *_act variants) and anirec_predict_workspace_bytes_w bytes */
int anirec_predict_grid_w(const float *U, const float *A, int32_t dim, int32_t n_anime, const int32_t *users,
                          int32_t n_users, const anirec_head *head_host, int32_t activation, float *out,
                          void *workspace, size_t workspace_bytes, void *stream);

/* The same grid on the matrix cores: rows are split x = hi + lo in fp16 and accumulated as
 * hi*hi + hi*lo + lo*hi by v_mfma_f32_32x32x16_f16.  Proven bound against exact arithmetic, for cosine c of the
 * normalised rows and S = sum |u_k a_k| <= 1: |dc| <= 3.2e-5 S (split 3 x 2^-22, 384 accumulation and 134
 * normalisation roundings of 2^-24 each), so |drating| <= max act' x (|hs| |dc| + 2^-23 (|c hs| + |hb| + |y|)) plus
 * the activation's own error — looser than 1e-5 once |hs| max act' > ~0.3.  Measured: within 1e-5 of the fp32 path
 * on the suite's heads, and within 2e-6 of fp64 on adversarial rows (tests/test_mfma_bounds_gpu.py). */
size_t anirec_predict_mfma_workspace_bytes(int32_t n_anime, int32_t n_users);
int anirec_predict_grid_mfma(const float *U, const float *A, int32_t n_anime, const int32_t *users,
                             int32_t n_users, const anirec_head *head_host, float *out,
                             void *workspace, size_t workspace_bytes, void *stream);
/* the epilogue of each activation is a fast form (hardware exp2 / log2 / rcp) within 1e-5 of the exact path */
int anirec_predict_grid_mfma_act(const float *U, const float *A, int32_t n_anime, const int32_t *users,
                                 int32_t n_users, const anirec_head *head_host, int32_t activation, float *out,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* Per query user: top-k anime by descending predicted rating among anime whose
 * watched bit is clear.  watched: optional [n_users][ceil(n_anime/32)] bitmask words.
 * (model_recs.py:144-155 candidate set, :396 ranking, :451-454 cut). */
int anirec_predict_topk(const float *U, const float *A, int32_t n_anime, const int32_t *users,
                        int32_t n_users, const anirec_head *head_host, const uint32_t *watched,
                        int32_t k, int32_t *out_idx, float *out_p, void *workspace,
                        size_t workspace_bytes, void *stream);
int anirec_predict_topk_act(const float *U, const float *A, int32_t n_anime, const int32_t *users,
                            int32_t n_users, const anirec_head *head_host, int32_t activation,
                            const uint32_t *watched, int32_t k, int32_t *out_idx, float *out_p, void *workspace,
                            size_t workspace_bytes, void *stream);
int anirec_predict_topk_w(const float *U, const float *A, int32_t dim, int32_t n_anime, const int32_t *users,
                          int32_t n_users, const anirec_head *head_host, int32_t activation,
                          const uint32_t *watched, int32_t k, int32_t *out_idx, float *out_p, void *workspace,
                          size_t workspace_bytes, void *stream);
/* anirec_predict_topk_act for ANY k >= 1 (k >= n_anime: a user's whole ranking), as anirec_cosine_topk_large.
 * workspace: anirec_predict_topk_large_workspace_bytes(n_anime, n_users, k) bytes. */
size_t anirec_predict_topk_large_workspace_bytes(int32_t n_anime, int32_t n_users, int32_t k);
int anirec_predict_topk_large_act(const float *U, const float *A, int32_t n_anime, const int32_t *users,
                                  int32_t n_users, const anirec_head *head_host, int32_t activation,
                                  const uint32_t *watched, int32_t k, int32_t *out_idx, float *out_p,
                                  void *workspace, size_t workspace_bytes, void *stream);
size_t anirec_predict_topk_large_workspace_bytes_w(int32_t n_anime, int32_t n_users, int32_t k, int32_t dim);
int anirec_predict_topk_large_w(const float *U, const float *A, int32_t dim, int32_t n_anime, const int32_t *users,
                                int32_t n_users, const anirec_head *head_host, int32_t activation,
                                const uint32_t *watched, int32_t k, int32_t *out_idx, float *out_p,
                                void *workspace, size_t workspace_bytes, void *stream);

/* Rank of held-out anime in a user's ranking, without the ranking: per target t = (target_row[t], target_anime[t]),
 * target_row indexing `users`, with p_j the predicted rating of users[target_row[t]] for anime j,
 *   out_rank[t] = #{ j != a_t : watched bit j of row target_row[t] clear and
 *                    (key(p_j) > key(p_t) or (key(p_j) == key(p_t) and j < a_t)) },   out_p[t] = p_{a_t}
 * key: larger rating first, NaN after every number, ties in ascending index — the order of anirec_predict_topk*.  The
 * target's own watched bit is ignored, so out_rank[t] is the position of a_t in the whole ranking
 * anirec_predict_topk_large_w(k >= n_anime) returns for that user under the same mask with bit a_t cleared, and
 * out_p[t] that list's rating, bit for bit (the same normalised rows, fma chain, head and activation).
 * dim: one of 32, 64, 128, 256.  watched: optional [n_users][ceil(n_anime/32)], as anirec_predict_topk.
 * *err_flag (device) becomes 1 on a target_row outside [0, n_users) or a target_anime outside [0, n_anime): that
 * target gets rank -1 and a NaN rating, nothing is read through it, the other targets are unaffected.
 * n_targets == 0 or n_users == 0: ANIREC_OK, nothing enqueued.  The counts of a target over slices of the anime
 * table meet in an integer atomic add: results are bit-reproducible.  Cost: 2 n_targets n_anime dim flops of the
 * fp32 chain, 8 bytes stored per target; no [n_targets, n_anime] matrix exists.
 * workspace: anirec_predict_rank_workspace_bytes(n_anime, n_users, n_targets, dim) bytes (the normalised rows). */
size_t anirec_predict_rank_workspace_bytes(int32_t n_anime, int32_t n_users, int32_t n_targets, int32_t dim);
int anirec_predict_rank(const float *U, const float *A, int32_t dim, int32_t n_anime, const int32_t *users,
                        int32_t n_users, const anirec_head *head_host, int32_t activation, const uint32_t *watched,
                        const int32_t *target_row, const int32_t *target_anime, int32_t n_targets, int32_t *out_rank,
                        float *out_p, int32_t *err_flag, void *workspace, size_t workspace_bytes, void *stream);

/* The same rank under ONE score vector shared by all users (a popularity baseline: score[j] = how often anime j was
 * rated): per target t = (target_row[t], target_anime[t]),
 *   out_rank[t] = #{ j != a_t : watched bit j of row target_row[t] clear and
 *                    (key(score[j]) > key(score[a_t]) or (key(score[j]) == key(score[a_t]) and j < a_t)) }
 * key as anirec_predict_rank: larger score first, NaN after every number, ties in ascending index.  The target's own
 * watched bit is ignored; bits at positions >= n_anime of a row's last word have no effect.
 * watched: optional [n_users][ceil(n_anime/32)].  *err_flag (device) is cleared by the call and becomes 1 on a
 * target_row outside [0, n_users) or a target_anime outside [0, n_anime): that target gets rank -1, nothing is read
 * through it, the other targets are unaffected.  n_anime < 1, a negative count, or a NULL score, target array,
 * out_rank or err_flag with n_targets > 0: ANIREC_EINVAL.  n_targets == 0: ANIREC_OK, nothing enqueued.  One wave
 * per target, no workspace, no atomics: bit-reproducible.  Cost: n_targets n_anime compares, 4 bytes per target. */
int anirec_score_rank(const float *score, int32_t n_anime, const uint32_t *watched, int32_t n_users,
                      const int32_t *target_row, const int32_t *target_anime, int32_t n_targets, int32_t *out_rank,
                      int32_t *err_flag, void *stream);

/* Watched bits of a rating list: bits[n_users][ceil(n_anime/32)] is zeroed, then bit (a & 31) of word a >> 5 of row u
 * is set for each of the n ratings (user_idx[i], anime_idx[i]) = (u, a); repeats are harmless.  The table
 * anirec_predict_topk* and anirec_predict_rank take as `watched`.  *err_flag (device) becomes 1 on an index out of
 * range; that rating sets nothing. */
int anirec_seen_bits(const int32_t *user_idx, const int32_t *anime_idx, int64_t n, int32_t n_users, int32_t n_anime,
                     uint32_t *bits, int32_t *err_flag, void *stream);

/* GROUP recommendations: one list for several users who watch together.  Group g has the members
 * e = group_offsets[g] .. group_offsets[g+1]-1 (CSR; c_g = their number); member e is user users[member_row[e]]
 * (member_row indexes `users`, as anirec_predict_rank's target_row).  A row listed twice counts as two members; a user
 * may belong to any number of groups.
 *   p_e[j]   the rating anirec_predict_grid_w writes for that user and anime j, bit for bit (the same
 *            tf.nn.l2_normalize rows, k-ordered fmaf chain from 0, head and activation)
 *   s_g[j]   the aggregate over the group's members, fp32, in member order, nothing contracted:
 *            ANIREC_GROUP_MEAN  s = p_0; s = s + p_i, i = 1 .. c-1; then s / (float)c, correctly rounded
 *            ANIREC_GROUP_MIN   a = p_0; for i >= 1: p_i NaN -> a = p_i; else a not NaN and p_i < a -> a = p_i
 *                               (least misery: a NaN sticks, of +-0 the earlier member stays)
 *            ANIREC_GROUP_MAX   the same with > (most pleasure)
 * Anime j is no candidate of group g if the watched bit j of any member is set (bits at positions >= n_anime have no
 * effect), if bit j of exclude[g] is set, or if p_i[j] < floor for any member (false for a NaN rating; floor =
 * -INFINITY switches the rule off).  The candidates are ranked by s_g in the order of anirec_predict_topk*: larger
 * first, +0 above -0, NaN after every number, ties in ascending index; any k >= 1 (k <= ANIREC_MAX_TOPK and above it
 * the two selects of anirec_predict_topk_w / _large_w, the same bits where they overlap); out_idx / out_score
 * [n_groups][k] are padded with -1 / NaN.  out_member_p (optional, [n_members][k]): out_member_p[e][s] =
 * p_e[out_idx[g][s]], NaN where the pick is -1; every element no valid group covers is NaN.  A one-member group
 * returns, in every mode, that user's anirec_predict_topk_large_w list bit for bit.
 * watched: optional [n_users][ceil(n_anime/32)], rows follow `users`; exclude: optional [n_groups][ceil(n_anime/32)].
 * *err_flag (device) is overwritten by the call; it becomes 1 on a member_row outside [0, n_users) or an offsets pair
 * that is negative, decreasing, past n_members or longer than max_members: that group's rows are -1 / NaN, nothing is
 * read through the bad value, the other groups are unaffected (should the pairs of valid groups overlap after such a
 * pair, the out_member_p rows they share hold either group's ratings).  An empty group gives -1 / NaN and no error.
 * max_members: an upper bound of the c_g, 1 .. ANIREC_GROUP_MAX_MEMBERS; it sizes the kernel's tiles and changes no
 * result.  A group's outputs depend on that group alone: not on the other groups, its position, max_members, the
 * workspace size or the run.  No atomics, no host synchronisation: graph-capturable.
 * A bad dim, activation or mode, a NaN floor, n_anime < 1, a negative count, k < 1, max_members out of range, or a
 * NULL U, A, head_host, group_offsets, out_idx, out_score, err_flag or workspace (users with n_users > 0, member_row
 * with n_members > 0) with n_groups > 0: ANIREC_EINVAL before anything is enqueued or written (0 from the size query
 * for those it can see).  n_groups == 0: ANIREC_OK, nothing enqueued.
 * workspace: may hold anything; Ah | Uh, then the select's fixed part and per group of a batch (at most 4096) a score
 * row, a mask row and the select's share.  anirec_group_topk_workspace_bytes sizes it; anything down to one group's
 * share runs the groups in smaller batches with the same results, less is ANIREC_EWORKSPACE.
 * Cost: 2 (slots) n_anime dim flops of the fp32 chain with slots = n_groups next_pow2(max_members) rounded up to 64,
 * 4 n_anime + n_anime / 8 bytes stored per group; no [n_members, n_anime] matrix exists. */
enum { ANIREC_GROUP_MEAN = 0, ANIREC_GROUP_MIN = 1, ANIREC_GROUP_MAX = 2 };
#define ANIREC_GROUP_MAX_MEMBERS 64
size_t anirec_group_topk_workspace_bytes(int32_t n_anime, int32_t n_users, int32_t n_groups, int32_t k, int32_t dim);
int anirec_group_topk(const float *U, const float *A, int32_t dim, int32_t n_anime, const int32_t *users,
                      int32_t n_users, const anirec_head *head_host, int32_t activation, const uint32_t *watched,
                      const int32_t *group_offsets, const int32_t *member_row, int32_t n_groups, int32_t n_members,
                      int32_t max_members, const uint32_t *exclude, int32_t mode, float floor, int32_t k,
                      int32_t *out_idx, float *out_score, float *out_member_p, int32_t *err_flag, void *workspace,
                      size_t workspace_bytes, void *stream);

/* FOLD-IN of new users: a user the model was not trained on (model_recs.py:373-394 reads the user's row out of the
 * trained table and has none) gets a row fitted to that user's own ratings with everything else frozen — the Keras
 * model of neural_network.py:66-106 with the anime table, Dense(1) and BatchNorm (inference mode) fixed and a fresh
 * one-row user embedding, model.fit full-batch on the user's ratings with Keras-2.12 Adam.
 * New user j holds ratings offsets[j] .. offsets[j+1]-1 of (anime_idx, rating) (CSR; n = their number; repeats count
 * as separate ratings; rating = the scaled target t).  Ah = A with rows scaled by 1/sqrt(max(sum a^2, 1e-12)) (the
 * train step's forward), hs, hb = the folded inference head (y = c*hs + hb), u starts at init[j], m = v = 0.  For
 * s = 1 .. steps, in fp32:
 *     ru = 1/sqrt(max(sum u^2, 1e-12));  uh = u*ru
 *     c_i = <uh, ah_i>;  y_i = fma(c_i, hs, hb);  p_i = act(y_i), g_i = dl/dy_i of ANIREC_ACT_* / ANIREC_LOSS_* above
 *     dc_i = (g_i / n) * hs
 *     grad = ru * sum_i dc_i (ah_i - c_i uh) + 2*l2*u
 *     m += (grad-m)*0.1; v += (grad*grad-v)*0.001; u -= (m*alpha[s-1])/(sqrt(v)+1e-7)      (the ADAM rule above:
 *                                                               correctly rounded sqrt and divide, nothing contracted)
 * alpha[s-1] = lr*sqrt(1-b2^s)/(1-b1^s), computed by the caller (device array).  out_rows[j] = u after the last step;
 * out_loss[j] = (1/n) sum_i l(p_i, t_i) + l2 * sum u^2 at that final row.  steps == 0: out_rows = init, out_loss the
 * loss there.  n == 0: out_rows[j] = init[j] bit for bit, out_loss[j] = NaN.
 * One workgroup per user, every step inside one launch, no float atomics: the partial sums of a user's list meet in a
 * fixed order that depends on that list alone, so a user's row and loss are the same bits run to run, whatever other
 * users share the call and wherever the user stands in it.
 * dim: one of 32, 64, 128, 256.  Bad dim / activation / loss, n_anime < 1, negative steps or n_new, a NULL pointer or
 * workspace_bytes < anirec_fold_in_workspace_bytes(n_anime, n_new, dim): ANIREC_EINVAL before anything is enqueued
 * (0 from the size query).  n_new == 0: ANIREC_OK, nothing enqueued.  anime_idx / rating may be NULL only when every
 * list is empty.  *err_flag (device) becomes 1 on an anime_idx outside [0, n_anime), a negative or decreasing
 * offsets pair, or a list of more than INT32_MAX ratings: that user's row and loss become NaN, nothing is read through
 * the bad value, the other users are unaffected (anirec_predict_rank's convention).  The call does not know how many
 * ratings anime_idx and rating hold (the ABI carries no count): the CALLER guarantees that every offset is at most
 * that number — an offset past it is read through like any other.  The workspace (the normalised anime rows) may hold anything on
 * entry; out_rows, out_loss and *err_flag are fully written. */
size_t anirec_fold_in_workspace_bytes(int32_t n_anime, int32_t n_new, int32_t dim);
int anirec_fold_in(const float *A, int32_t dim, int32_t n_anime, const anirec_head *head_host, int32_t activation,
                   int32_t loss, float l2, const int64_t *offsets, const int32_t *anime_idx, const float *rating,
                   int32_t n_new, const float *init, const float *alpha, int32_t steps, float *out_rows,
                   float *out_loss, int32_t *err_flag, void *workspace, size_t workspace_bytes, void *stream);

/* FOLD-IN WITH THE LIST SPLIT ACROSS WORKGROUPS: the fit above for a few rows with long lists — a new ANIME that
 * known users have rated, fitted against the frozen user table (the prediction depends on the two rows through their
 * cosine alone, so the tables swap roles).  T [n_table][dim] is the frozen table, idx its rows; every other argument,
 * the definition of a step, the n == 0 and steps == 0 cases, the argument checks and the caller's guarantee on the
 * offsets are anirec_fold_in's.  What differs is the order of the sums.  Row r's list is cut into
 * ceil(n_r / ANIREC_FOLD_CHUNK) chunks, chunk j holding ratings [1024 j, min(n_r, 1024 (j+1))) of the list.  Per step
 *     partial_j = the sum over chunk j's ratings of dc_i (ah_i - c_i uh), in anirec_fold_in's order over the chunk
 *                 (lane group g takes ratings g, g + kNG, ... of the chunk, the groups added in order 0 .. kNG-1;
 *                 dc_i = (g_i / n_r) * hs with the row's whole n_r), and the chunk's loss sum the same way
 *     grad      = ru * (((partial_0 + partial_1) + partial_2) + ...) + 2*l2*u        (ascending chunk order)
 * and out_loss = (((l_0 + l_1) + ...) / n_r) + l2 * sum u^2.  No atomics; a step is two plain launches (one workgroup
 * per chunk, then one lane group per row), 2 steps + 4 launches a call, no grid-wide wait.  Two consequences:
 *   - a row's bits depend on its own list, its start row and ANIREC_FOLD_CHUNK alone: not on the other rows, its
 *     position in the call, or the run;
 *   - a list of at most ANIREC_FOLD_CHUNK ratings gives the bits of anirec_fold_in, row and loss.
 * The caller passes the chunk map (device arrays): chunk_offsets[n_new + 1] = the prefix sums of the rows' chunk
 * counts (a row with a bad offsets pair counts 0 chunks), chunk_row[n_chunks] = the row of each chunk, n_chunks =
 * chunk_offsets[n_new].  chunk_row may be NULL when n_chunks == 0.  Every offsets pair, every index and the map are
 * validated before anything is gathered: a bad pair or index poisons its own row (NaN row and loss, *err_flag = 1),
 * the others are unaffected; a map that is not the one the offsets define makes EVERY row and loss NaN with
 * *err_flag = 1, and nothing is read through it.
 * workspace: anirec_fold_in_split_workspace_bytes(n_table, n_new, n_chunks, dim) bytes (the normalised table, m, v,
 * one partial row and loss per chunk, the row flags); it may hold anything on entry.  0 from the size query and
 * ANIREC_EINVAL before anything is enqueued for a bad argument (n_chunks < 0 among them). */
size_t anirec_fold_in_split_workspace_bytes(int32_t n_table, int32_t n_new, int32_t n_chunks, int32_t dim);
int anirec_fold_in_split(const float *T, int32_t dim, int32_t n_table, const anirec_head *head_host, int32_t activation,
                         int32_t loss, float l2, const int64_t *offsets, const int32_t *idx, const float *rating,
                         int32_t n_new, const int32_t *chunk_offsets, const int32_t *chunk_row, int32_t n_chunks,
                         const float *init, const float *alpha, int32_t steps, float *out_rows, float *out_loss,
                         int32_t *err_flag, void *workspace, size_t workspace_bytes, void *stream);

/* DIVERSIFIED LISTS — greedy maximal-marginal-relevance (MMR) re-rank.  model_recs.py:373-456 cuts a user's list by
 * predicted rating alone, and the rating sees an anime only through the cosine of its row with the user's: rows that
 * nearly coincide (the seasons, specials and movies of one franchise) enter a top-k together.  Here a list of n_cand
 * candidates (anirec_predict_topk*'s output for k = the pool) becomes a list of k picks, each pick trading a
 * candidate's score against its similarity to what is already picked.
 * What [n_rows][dim] = the unit rows anirec_rownorm_w writes; list l holds the candidates cand_idx[l][0 .. n_cand)
 * (rows of What; -1 = an empty slot) with relevance cand_score[l][.].  All arithmetic is fp32, nothing is contracted
 * into an fma, oml = 1.0f - lambda.
 *     absent   a candidate whose index is -1, whose score is NaN, or whose What row holds a non-finite value (a zero
 *              row normalises to NaN); every other candidate is present.  An index that appears twice is two candidates.
 *     sim(i,j) the k-ordered chain s = fmaf(What[a_i][t], What[a_j][t], s), t = 0 .. dim-1, from s = 0: the chain of
 *              anirec_cosine_scores_w, the same bits
 *     pen_i    0 while nothing is picked; after the first pick sim(i, first), then the larger of pen_i and sim(i, j)
 *              for each later pick j (it may be negative; a NaN sim, which unit rows cannot give, replaces nothing)
 *     val_i    (lambda * score_i) - (oml * pen_i): each product rounded, then the difference
 *     pick s   = 0 .. k-1: among the present, unpicked candidates the one with the largest val; ties (-0 == +0) go to
 *              the lowest position in the list; +-inf scores are ordinary numbers; a NaN val (inf - inf, 0 * inf)
 *              sorts after every number.  The pick at position pos writes
 *                  out_idx[l][s] = cand_idx[l][pos], out_pos[l][s] = pos, out_score[l][s] = cand_score[l][pos],
 *                  out_pen[l][s] = pen_pos at that moment (0 for the first pick)
 * With fewer than k present candidates the rest of the row is -1 / -1 / NaN / NaN.  lambda == 1 returns the first k
 * present candidates in (score descending, position ascending) order.
 * One workgroup per list, every pick inside one launch, the candidates' rows staged once in LDS (dim * n_cand <=
 * 32768 floats: anirec_mmr_max_cand(dim) = 32768 / dim = 1024, 512, 256, 128 candidates; 0 for a bad dim); a pick
 * costs n_cand chains against the picked row, the n_cand x n_cand matrix is never formed.  No workspace, no atomics,
 * stream-ordered and graph-capturable.  A list's outputs depend on that list alone: not on the other lists, on its
 * position in the call, or on the run.
 * Bad dim, n_rows < 1, a negative count, k < 1 or k > n_cand, n_cand > anirec_mmr_max_cand(dim), lambda outside [0, 1]
 * or NaN, a NULL pointer with n_lists > 0: ANIREC_EINVAL before anything is enqueued or written.  n_lists == 0:
 * ANIREC_OK, nothing enqueued.  Otherwise every element of the four outputs and *err_flag (device) is written:
 * *err_flag becomes 1 on a candidate index below -1 or at or above n_rows (0 without one): that list's whole output
 * is -1 / -1 / NaN / NaN, nothing is read through the bad index, the other lists are unaffected (anirec_predict_rank's
 * convention). */
size_t anirec_mmr_max_cand(int32_t dim);
int anirec_mmr_rerank(const float *What, int32_t dim, int32_t n_rows, const int32_t *cand_idx, const float *cand_score,
                      int32_t n_lists, int32_t n_cand, int32_t k, float lambda, int32_t *out_idx, int32_t *out_pos,
                      float *out_score, float *out_pen, int32_t *err_flag, void *stream);

/* LIST EVALUATION — the pairwise similarity structure of many lists at once: what a re-ranked list (anirec_mmr_rerank)
 * buys is a property of the list itself, how alike its rows are.  What [n_rows][dim] = the unit rows anirec_rownorm_w
 * writes; list_idx [n_lists][k] = rows of What, -1 = an empty slot: what anirec_predict_topk* and anirec_mmr_rerank
 * write.  Both outputs are [n_lists][k] fp32.  All arithmetic is fp32 and nothing is contracted.
 *     present  slot s is present when list_idx[l][s] != -1; an index that appears twice is two slots
 *     sim(s,j) the k-ordered chain acc = fmaf(What[a_s][t], What[a_j][t], acc), t = 0 .. dim-1, from 0: the chain of
 *              anirec_cosine_scores_w and anirec_mmr_rerank's sim, the same bits
 *     a present slot s with the earlier present slots j1 < j2 < ... (ascending position):
 *              out_sim_sum[l][s] = ((0 + sim(s,j1)) + sim(s,j2)) + ..., fp32 adds in that order
 *              out_sim_max[l][s] = anirec_mmr_rerank's pen rule: sim(s,j1), then replaced by sim(s,j) for each later j
 *                                  with sim(s,j) > the current value (a NaN replaces nothing)
 *              both 0.0f with no earlier present slot
 *     an absent slot: both are the NaN 0x7FC00000
 * Rows with non-finite values are not special-cased: their NaN propagates by the rules above.  So for the out_idx of an
 * anirec_mmr_rerank call out_sim_max holds that call's out_pen, bit for bit, padding included.
 * A group of lanes per list (one wave for a short list, a workgroup beyond), the list's rows staged once in LDS (dim * k
 * <= 32768 floats: k <= anirec_mmr_max_cand(dim)), the pairs of the triangle dealt evenly over the lanes.  No workspace,
 * no atomics, stream-ordered and graph-capturable.  A list's outputs depend on that list alone.
 * Bad dim, n_rows < 1, a negative count, k < 1, k > anirec_mmr_max_cand(dim), a NULL pointer with n_lists > 0:
 * ANIREC_EINVAL before anything is enqueued or written.  n_lists == 0: ANIREC_OK, nothing enqueued.  Otherwise every
 * element of both outputs and *err_flag (device) is written: *err_flag becomes 1 on an index below -1 or at or above
 * n_rows (0 without one): that list's two output rows are all NaN, nothing is read through the bad index, the other
 * lists are unaffected (anirec_predict_rank's convention). */
int anirec_list_similarity(const float *What, int32_t dim, int32_t n_rows, const int32_t *list_idx, int32_t n_lists,
                           int32_t k, float *out_sim_max, float *out_sim_sum, int32_t *err_flag, void *stream);

/* CALIBRATED LISTS — greedy re-rank towards the user's own category proportions (Steck, "Calibrated recommendations",
 * RecSys 2018, with total variation in place of KL).  A rating head amplifies the majority taste: favourites that are
 * 70 % action and 30 % romance give a top-10 that is all action.  Here a list of n_cand candidates becomes a list of k
 * picks, each pick trading a candidate's score against the miscalibration of the list with that candidate added.
 * cat_bits [n_rows][cw] uint32, cw = ceil(n_cat / 32), 1 <= n_cat <= 128: bit c of row a set iff anime a carries
 * category c (anirec_fave_profile's layout; bits at positions >= n_cat of the last word are ignored).  List l holds
 * the candidates cand_idx[l][0 .. n_cand) (rows of cat_bits; -1 = an empty slot) with relevance cand_score[l][.] and the
 * profile profile[l][0 .. n_cat): one row of anirec_fave_profile's counts.  Tokens are unweighted on both sides: an
 * anime with three categories adds three tokens (the word-cloud semantics of get_genres, and what the profile counts).
 *     present  a candidate whose index is >= 0 and whose score is not NaN; b_i its category bits, pop_i their number.
 *              An index that appears twice is two candidates.
 *     state    q_c = the number of picked candidates that carry category c, Q = sum q_c, P = sum p_c
 *     pen_i    the total variation distance of the two token distributions for the list extended by candidate i,
 *              Q' = Q + pop_i, q' = q + b_i:
 *                  0.0f when P == 0 (nothing to calibrate to); otherwise 1.0f when Q' == 0 (the list says nothing);
 *                  otherwise num = sum_c |p_c Q' - q'_c P|, den = 2 P Q', both int64, and
 *                  pen = (float)((double)num / (double)den)
 *              With p_c <= 2^24, n_cat <= 128 and n_cand <= 1024: P <= 2^31, Q' <= 2^17, every term < 2^42 and
 *              num <= den <= 2^49 < 2^53: both conversions to double are exact, the division and the conversion to fp32
 *              are each correctly rounded, and no sum depends on its order.
 *     val_i    (omc * score_i) - (calibration * pen_i) in fp32, omc = 1.0f - calibration: each product rounded, then
 *              the difference, nothing contracted into an fma
 *     pick s   = 0 .. k-1: among the present, unpicked candidates the one with the largest val, in anirec_mmr_rerank's
 *              order: ties (-0 == +0) go to the lowest position, a NaN val sorts after every number.  The pick at
 *              position pos is added to q and writes
 *                  out_idx[l][s] = cand_idx[l][pos], out_pos[l][s] = pos, out_score[l][s] = cand_score[l][pos],
 *                  out_pen[l][s] = pen_pos at that moment: the miscalibration of the list INCLUDING pick s
 * With fewer than k present candidates the rest of the row is -1 / -1 / NaN / NaN.  The result is greedy: its first k'
 * columns are the result for k' < k.  calibration == 0 returns the first k present candidates in (score descending,
 * position ascending) order.
 * One group of lanes per list (a wave up to 256 candidates, a workgroup of four beyond), every pick inside one launch;
 * anirec_calibrate_max_cand() = 1024 candidates at most.  No workspace, no atomics, stream-ordered and
 * graph-capturable.  A list's outputs depend on that list alone.
 * n_cat outside 1 .. 128, n_rows < 1, a negative count, k < 1 or k > n_cand, n_cand > anirec_calibrate_max_cand(),
 * calibration outside [0, 1] or NaN, a NULL pointer with n_lists > 0: ANIREC_EINVAL before anything is enqueued or
 * written.  n_lists == 0: ANIREC_OK, nothing enqueued.  Otherwise every element of the four outputs and *err_flag
 * (device) is written: *err_flag becomes 1 on a bad list (0 without one) — a candidate index below -1 or at or above
 * n_rows, or a profile entry that is negative or above 2^24: that list's whole output is -1 / -1 / NaN / NaN, nothing
 * is read through its indices, the other lists are unaffected. */
size_t anirec_calibrate_max_cand(void);
int anirec_calibrate_rerank(const uint32_t *cat_bits, int32_t n_rows, int32_t n_cat, const int32_t *cand_idx,
                            const float *cand_score, const int32_t *profile, int32_t n_lists, int32_t n_cand, int32_t k,
                            float calibration, int32_t *out_idx, int32_t *out_pos, float *out_score, float *out_pen,
                            int32_t *err_flag, void *stream);

/* The miscalibration of lists a caller holds, by the definition above: lists [n_lists][k] = rows of cat_bits, -1 = an
 * empty slot (skipped; an index that appears twice is two slots), 1 <= k <= anirec_calibrate_max_cand();
 * profile [n_lists][n_cat].  With q_c and Q counted over the list's present slots:
 *     P == 0:     out_num[l] = 0, out_den[l] = 1, out_pen[l] = 0.0f
 *     else Q == 0: out_num[l] = 1, out_den[l] = 1, out_pen[l] = 1.0f
 *     else        out_num[l] = sum_c |p_c Q - q_c P|, out_den[l] = 2 P Q, out_pen[l] = (float)((double)num / (double)den)
 * So for the first s + 1 columns of an anirec_calibrate_rerank call's out_idx and the same profile, out_pen is that
 * call's out_pen[l][s], bit for bit.  One wave per list, no workspace, no atomics, graph-capturable.  Refusals as above
 * (n_cat, n_rows, counts, k, NULL pointers); a bad list (an index below -1 or at or above n_rows, a profile entry that
 * is negative or above 2^24) gets -1 / -1 / NaN and *err_flag = 1, nothing read through its indices. */
int anirec_list_calibration(const uint32_t *cat_bits, int32_t n_rows, int32_t n_cat, const int32_t *lists,
                            const int32_t *profile, int32_t n_lists, int32_t k, int64_t *out_num, int64_t *out_den,
                            float *out_pen, int32_t *err_flag, void *stream);

/* EXPLAINED LISTS — why an anime is in a list: a predicted rating sees an anime only through the cosine of two rows,
 * so "recommended because you rated X, Y, Z" has an answer inside the model: the anime of the user's own history whose
 * rows lie closest to the listed one, each weighted by what the user gave it.
 * What [n_rows][dim] = the unit rows anirec_rownorm_w writes; list_idx [n_lists][k] = rows of What, -1 = an empty slot
 * (what anirec_predict_topk*, anirec_mmr_rerank and anirec_group_topk write).  List l's history is entries
 * hist_offsets[l] .. hist_offsets[l+1]-1 of (hist_idx, hist_weight): anirec_fold_in's CSR, with the same CALLER's
 * guarantee on the offsets (the ABI carries no count); a repeated anime is two entries.  The three outputs are
 * [n_lists][k][m].  All arithmetic is fp32 and nothing is contracted.
 *     sim(s,i)     the k-ordered chain acc = fmaf(What[a_s][t], What[h_i][t], acc), t = 0 .. dim-1, from 0: the chain of
 *                  anirec_cosine_scores_w, anirec_mmr_rerank and anirec_list_similarity, the same bits
 *     contrib(s,i) hist_weight[i] * sim(s,i): one rounded product
 *     order        for a present slot s (list_idx != -1) the history entries by contrib descending, ties (==, so that
 *                  -0 == +0; twin rows and repeated entries do tie) to the lowest history position; +-inf are ordinary
 *                  numbers; an entry whose contrib is NaN (a zero row normalised to NaN, 0 * inf, a NaN weight) is
 *                  never picked.  A history entry equal to the listed anime is not special-cased.
 *     rank r < m   out_pos[l][s][r] = the entry's position within the list's own history (0-based),
 *                  out_sim[l][s][r] = sim, out_contrib[l][s][r] = contrib
 * With fewer than m pickable entries the rest of the slot's row is -1 / NaN / NaN (the NaN 0x7FC00000); an absent slot
 * is -1 / NaN / NaN throughout.  The order is total, so the result does not depend on how the history is split over
 * lanes, waves or passes, and a list's outputs depend on that list alone: not on the other lists, its position in the
 * call, or the run.
 * One workgroup per list, the list's rows staged once in LDS, the history streamed through a second LDS image in tiles
 * of anirec_explain_tile(dim, k) entries (a history of any length runs through that loop), each slot's running top-m in
 * registers.  anirec_explain_max_k(dim) = min(128, 16384 / dim) = 128, 128, 128, 64 slots; both queries return 0 for a
 * bad argument.  No workspace, no atomics, stream-ordered and graph-capturable.
 * Bad dim, n_rows < 1, a negative count, k < 1 or k > anirec_explain_max_k(dim), m < 1 or m > ANIREC_EXPLAIN_MAX_M, a
 * NULL pointer with n_lists > 0 (hist_idx / hist_weight may be NULL only when every history is empty): ANIREC_EINVAL
 * before anything is enqueued or written.  n_lists == 0: ANIREC_OK, nothing enqueued.  Otherwise every element of the
 * three outputs and *err_flag (device) is written: *err_flag becomes 1 on a list index below -1 or at or above n_rows,
 * a history index outside [0, n_rows), a negative or decreasing offsets pair, or a history of more than INT32_MAX
 * entries (0 without one): that list's whole output is -1 / NaN / NaN, nothing is read through the bad value (every
 * index of the list and its history is validated before any row is gathered), the other lists are unaffected
 * (anirec_predict_rank's convention). */
#define ANIREC_EXPLAIN_MAX_M 8
size_t anirec_explain_max_k(int32_t dim);
size_t anirec_explain_tile(int32_t dim, int32_t k);
int anirec_explain_lists(const float *What, int32_t dim, int32_t n_rows, const int32_t *list_idx, int32_t n_lists,
                         int32_t k, const int64_t *hist_offsets, const int32_t *hist_idx, const float *hist_weight,
                         int32_t m, int32_t *out_pos, float *out_sim, float *out_contrib, int32_t *err_flag,
                         void *stream);

/* CLUSTERED TABLES — spherical k-means (Lloyd's algorithm on unit rows, the cosine as similarity) on an embedding table:
 * the view of the table as a whole that the per-row calls above cannot give.  Exact and order-free: the result does not
 * depend on how the rows are dealt to lanes, waves or workgroups, and a NumPy restatement reproduces it bit for bit.
 * What [n_rows][dim] = the unit rows anirec_rownorm_w writes; C [k][dim] = the centroids; dim one of 32, 64, 128, 256.
 *   the assign rule
 *     sim(i,c)    the k-ordered chain acc = fmaf(What[i][t], C[c][t], acc), t = 0 .. dim-1, from 0: the chain of
 *                 anirec_cosine_scores_w, the same bits; nothing is contracted beyond it
 *     usable row  every element finite and |x| <= 2; an unusable row (a zero row normalised to NaN) gets assignment -1
 *                 and sim NaN (0x7FC00000) and contributes to no centroid
 *     pick        for a usable row the centroid with the largest sim; ties (==, so that -0 == +0) to the lowest c; a
 *                 NaN sim is never picked; +-inf are ordinary numbers; no pickable centroid: -1 / NaN.  A row's pick
 *                 depends on that row and C alone.
 *   the update rule
 *     q(x)        llrint((double)x * 2^30): the product is exact, the rounding to nearest even
 *     S_c[t]      the sum of q(What[i][t]) over the rows assigned to c, as int64: a sum of integers, its bits do not
 *                 depend on order (2^31 rows of |x| <= 2 stay inside int64); cnt_c = the number of those rows
 *     cnt_c > 0   d_t = (double)S_c[t] (rounded to nearest even); nn = the chain over ascending t from 0.0 of a rounded
 *                 fp64 multiply d_t * d_t and a rounded fp64 add (no fma); with nn > 0: C[c][t] = (float)(d_t / sqrt(nn)),
 *                 IEEE fp64 sqrt and divide, one rounding to fp32
 *     cnt_c == 0 or nn == 0: the centroid keeps its bits (a NaN centroid, which nothing is ever assigned to, included)
 *   the fit loop   a_0 = -2 everywhere.  Iteration j = 1 .. max_iter: assign with the current C -> a_j; changed_j =
 *                 #{i : a_j[i] != a_(j-1)[i]}; changed_j == 0: stop, C untouched, converged; otherwise update C.  After
 *                 max_iter iterations without a stop one last assign pass is made with the final C.  So out_assign,
 *                 out_sim and out_count [k] (= cnt of out_assign) always belong to the returned C.
 *                 out_info = {iterations run (the j of the stop, or max_iter), converged 0/1}.
 * anirec_kmeans_assign is the assign rule alone (rows of any table against a given clustering).  The centroids are staged
 * in LDS anirec_kmeans_tile(dim) = 32768 / dim at a time (0 for a bad dim); a larger k runs as passes over tiles with the
 * running best kept per row, and the pick order is total, so the tiling cannot change a bit.
 * anirec_kmeans_fit enqueues all max_iter iterations at once, plain launches only, no host read-back, no cooperative
 * grid: stream-ordered and graph-capturable; once converged the remaining launches return on a device flag.  Integer
 * atomics only.  ws: anirec_kmeans_workspace_bytes(n_rows, k, dim) bytes (0 for a bad argument), 8-byte aligned; the
 * result does not depend on what it held before the call.
 * Bad dim, n_rows < 1, k < 1 or k > ANIREC_KMEANS_MAX_K, max_iter < 1 or max_iter > 1000, a NULL pointer, ws_bytes too
 * small: ANIREC_EINVAL before anything is enqueued or written.  Otherwise every element of every output is written. */
#define ANIREC_KMEANS_MAX_K 4096
size_t anirec_kmeans_tile(int32_t dim);
int anirec_kmeans_assign(const float *What, int32_t dim, int32_t n_rows, const float *C, int32_t k,
                         int32_t *out_assign, float *out_sim, void *stream);
size_t anirec_kmeans_workspace_bytes(int32_t n_rows, int32_t k, int32_t dim);
int anirec_kmeans_fit(const float *What, int32_t dim, int32_t n_rows, float *C_inout, int32_t k, int32_t max_iter,
                      int32_t *out_assign, float *out_sim, int32_t *out_count, int32_t *out_info,
                      void *ws, size_t ws_bytes, void *stream);

/* MAPPED TABLES — exact t-SNE: a two-dimensional map of an embedding table from its neighbour graph.  All pairs per
 * iteration, exact and order-free: the result is a function of (Y0, the CSR, the parameters) alone, it does not depend on
 * lanes, waves, j_splits or the order atomics land in, and a NumPy restatement reproduces every bit of Y, V and G after
 * any number of iterations.
 * Y [n][2] fp32 = the coordinates.  The affinities: a symmetric sparse matrix in CSR, offsets int64 [n + 1], idx int32,
 * val fp32 = P'_ij = p(j|i) + p(i|j) in [0, 2]; the attraction uses P' / (2 n) (the values stay in P' units: p itself,
 * about 1 / (n k), would drown in any fixed-point scale).  V, G [n][2] fp64 = velocity and gains.
 *   out row      a row with a coordinate that is not finite or above 2^60 in magnitude.  It takes part in no pair, as i
 *                or as j, stored or not: all its sums are 0 and it adds nothing to another row's sums or to Z.  Bit 0
 *                of out_info is raised.
 *   pair chain   for i != j, both in (excluded by index, not by distance: duplicate points give q = 1, count in Z and
 *                exert no force).  fp32, every operation rounded on its own, nothing contracted into an fma:
 *                dx = xi - xj, dy = yi - yj, d2 = dx*dx + dy*dy, q = 1 / (1 + d2) (IEEE divide), w = q*q.
 *   integer terms  S = 2^30; I(p) = rint(p * S): the product is exact, the rounding to the nearest even integer.
 *                Z     += I(q)           over every ordered pair (i, j)
 *                Rx_i  += I(w*dx),  Ry_i += I(w*dy)
 *                for a stored pair with a = val*q:  Ax_i += I(a*dx),  Ay_i += I(a*dy)
 *   bounds       q <= 1; |w*dx| <= 3 sqrt(3) / 16 < 0.33; |a*dx| <= 2 * 1/2 = 1 (a few fp32 roundings above it at
 *                most): every term fits an int32, a row sum stays inside int64 for any n < 2^31.  With coordinates up
 *                to 2^60, d2 <= 2^121 is finite and no term is a NaN: no input reaches a conversion that is not defined.
 *   Z            does NOT fit int64 (n^2 terms of up to 2^30): it is the exact integer sum in two words, out_z =
 *                {low, high} uint64, Z = high * 2^64 + low.  Z = 0 is possible (every point farther than 2^15.5 from
 *                every other); the repulsive term is then 0.
 *   stored pairs  an entry with idx outside 0 .. n-1 or idx == i, and every entry of a row whose offsets are not
 *                0 <= offsets[i] <= offsets[i+1] <= nnz, contributes 0 and raises bit 2; an entry whose val is not in
 *                [0, 2] (a NaN included) contributes 0 and raises bit 1.  Nothing is read through a bad value.
 *   update       iteration t = 0 .. iters-1, every row and coordinate on its own, fp64, each operation correctly rounded
 *                and none contracted.  e = exaggeration and momentum m = 0.5 while t < exag_iters, then e = 1, m = 0.8.
 *                Ad, Rd = (double) of the int64 sums; Zd = (double)high * 2^64 + (double)low (two roundings to nearest
 *                even, one rounded add)
 *                att  = (e * Ad) / (2^31 * n)              rep = Zd > 0 ? Rd / Zd : 0
 *                grad = 4 * (att - rep)
 *                g    = sgn(grad) != sgn(v) ? g + 0.2 : g * 0.8, then max(g, 0.01)   (sgn in {-1, 0, 1})
 *                v    = m * v - (lr * g) * grad
 *                y    = (float)((double)y + v)
 *                from v = 0, g = 1.  All rows move at once: every sum of iteration t is taken at the coordinates
 *                iteration t - 1 left.  No recentring.
 * anirec_tsne_forces: the integer sums at the given Y: out_rx, out_ry, out_ax, out_ay int64 [n], out_z uint64 [2],
 * out_info int32 [1]; no workspace.  anirec_tsne_fit: Y_inout moves by `iters` iterations; out_V, out_G [n][2] fp64 and
 * out_info are written.  One init kernel, then iters x (forces, attract + update), plain launches enqueued at once on
 * `stream`: no host read-back, no cooperative grid, no second stream; integer vector atomics only.  The all-pairs kernel
 * stages anirec_tsne_tile() j points in LDS at a time and splits the j range over j_splits workgroups a block of rows
 * (0 = the library's choice, at most 1024); no bit depends on it.  ws: anirec_tsne_workspace_bytes(n_rows, iters) bytes
 * (0 for a bad argument), 8-byte aligned; the call zeroes it, and the result does not depend on what it held.
 * n_rows < 1 or above ANIREC_TSNE_MAX_ROWS, iters < 1 or above ANIREC_TSNE_MAX_ITER, exag_iters < 0, nnz < 0, j_splits
 * outside 0 .. 1024, exaggeration not in (0, 1e6] or lr not in (0, 1e9] (a NaN included), a NULL pointer (idx and val
 * may be NULL with nnz == 0), ws_bytes too small or ws misaligned: ANIREC_EINVAL before anything is enqueued or written.
 * offsets is device memory: that it rises from 0 to nnz is the caller's to check; a row that breaks it is handled as
 * above. */
#define ANIREC_TSNE_MAX_ROWS 1048576
#define ANIREC_TSNE_MAX_ITER 4096
size_t anirec_tsne_tile(void);
size_t anirec_tsne_workspace_bytes(int32_t n_rows, int32_t iters);
int anirec_tsne_forces(const float *Y, int32_t n_rows, const int64_t *offsets, const int32_t *idx, const float *val,
                       int64_t nnz, int32_t j_splits, int64_t *out_rx, int64_t *out_ry, int64_t *out_ax, int64_t *out_ay,
                       uint64_t *out_z, int32_t *out_info, void *stream);
int anirec_tsne_fit(float *Y_inout, int32_t n_rows, const int64_t *offsets, const int32_t *idx, const float *val,
                    int64_t nnz, int32_t iters, int32_t exag_iters, double exaggeration, double lr, int32_t j_splits,
                    double *out_V, double *out_G, int32_t *out_info, void *ws, size_t ws_bytes, void *stream);

/* ITEM-kNN FROM CO-OCCURRENCE: "people who liked this also liked ...", and the baseline a neural model is judged by.
 * No model takes part.  item_bits is [n_items][ceil(n_users/32)] uint32: bit (u & 31) of word u >> 5 of row i is set
 * when user u liked item i — exactly what anirec_seen_bits writes when it is called with the two index columns swapped
 * (user_idx := the item column, anime_idx := the user column, n_users := n_items, n_anime := n_users); there is no
 * other builder.  Bits at positions >= n_users of a row's last word may hold anything and have no effect.
 *
 * anirec_cooc_scores: one similarity row per query item q = queries[t], against every item j:
 *   pop[i]   the popcount of row i over the valid bits
 *   c(q,j)   the popcount of row_q & row_j over the valid bits
 *   den      fp64, every operation one IEEE rounding, nothing contracted:
 *            ANIREC_COOC_COSINE      sqrt((double)pop_q * (double)pop_j) + shrink
 *            ANIREC_COOC_JACCARD     (double)(int64)(pop_q + pop_j - c) + shrink
 *            ANIREC_COOC_CONFIDENCE  (double)pop_q + shrink                            (P(j | q))
 *   sim      c >= max(1, min_support) ? (float)((double)c / den) : +0.0f    (den > 0 whenever c > 0)
 *   out_sim [nq][n_items] = sim; out_count (optional) [nq][n_items] = c; out_pop (optional) [n_items] = pop;
 *   out_excl (optional) [nq][ceil(n_items/32)]: bit j of row t set iff c < max(1, min_support) or j == q — the mask
 *   rows anirec_rows_topk takes as wbits; bits at positions >= n_items are clear.
 * A query outside [0, n_items) raises *err_flag (device; overwritten by the call) to 1: its rows are NaN / -1 / every
 * bit j < n_items set, nothing is read through it, the other queries are unaffected.  A query may repeat.  A query's
 * rows depend on that query and the bits alone: not on nq, its position in `queries` or the launch shape.  Every count
 * is a sum of integers, so the call is bit-reproducible.  A 256-thread workgroup owns 64 queries x 64 keys and stages
 * anirec_cooc_chunk_words() user words of both row sets in LDS per pass.
 * shrink must be finite and >= 0, min_support >= 0, n_users >= 1, n_items >= 1, measure one of the three; those, a
 * negative nq or a NULL item_bits, queries, out_sim, err_flag or ws with nq > 0: ANIREC_EINVAL before anything is
 * enqueued or written.  nq == 0: ANIREC_OK, nothing enqueued.  ws: anirec_cooc_workspace_bytes(n_items, nq) bytes (0
 * for a bad argument; the pop vector), less is ANIREC_EWORKSPACE; the result does not depend on what it held.
 * Stream-ordered plain launches, no host read-back: graph-capturable.
 * Cost: nq n_items ceil(n_users/32) word pairs of one v_and and one accumulating popcount each. */
enum { ANIREC_COOC_COSINE = 0, ANIREC_COOC_JACCARD = 1, ANIREC_COOC_CONFIDENCE = 2 };
size_t anirec_cooc_chunk_words(void);
size_t anirec_cooc_workspace_bytes(int32_t n_items, int32_t nq);
int anirec_cooc_scores(const uint32_t *item_bits, int32_t n_items, int32_t n_users, const int32_t *queries, int32_t nq,
                       int32_t measure, double shrink, int32_t min_support, float *out_sim, int32_t *out_count,
                       uint32_t *out_excl, int32_t *out_pop, int32_t *err_flag, void *ws, size_t ws_bytes,
                       void *stream);

/* The exact select over score rows the caller already holds: scores [nq][ld] fp32 (ld >= n; the first n of a row
 * count), any k >= 1.  Item j is no candidate of query t if j == self[t] (optional [nq]; -1 = none), keep[j] == 0
 * (optional [n] bytes) or bit j of wbits[t] is set (optional [nq][ceil(n/32)]; bits at positions >= n have no effect).
 * The order is that of anirec_predict_topk*: larger first, +0 above -0, NaN after every number, ties in ascending
 * index; out_idx / out_score [nq][k] are padded with -1 / NaN, out_score holds the row's own bits.  k <=
 * ANIREC_MAX_TOPK and above it run the two selects of anirec_predict_topk_w / _large_w exactly as anirec_group_topk
 * does (the same bits where they overlap).  n < 1, nq < 0, k < 1, ld < n, or a NULL scores, out_idx, out_score or
 * workspace with nq > 0: ANIREC_EINVAL before anything is enqueued.  nq == 0: ANIREC_OK.
 * workspace: may hold anything; anirec_rows_topk_workspace_bytes(n, nq, k) sizes it (0 for a bad argument): the
 * select's fixed part and per query of a batch (at most 4096) the select's share.  Anything down to one query's share
 * runs smaller batches with the same results, less is ANIREC_EWORKSPACE.  Graph-capturable. */
size_t anirec_rows_topk_workspace_bytes(int32_t n, int32_t nq, int32_t k);
int anirec_rows_topk(const float *scores, int64_t ld, int32_t n, int32_t nq, const int32_t *self, const uint8_t *keep,
                     const uint32_t *wbits, int32_t k, int32_t *out_idx, float *out_score, void *workspace,
                     size_t workspace_bytes, void *stream);

/* anirec_score_rank with one score row per user: score(t) = scores + (size_t)target_row[t] * ld, otherwise the same
 * key, tie rule, watched semantics and error rule (target_row outside [0, n_users) raises the flag before anything is
 * read through it).  ld == 0 is anirec_score_rank bit for bit; any other ld must be >= n_anime (ANIREC_EINVAL).  One
 * wave per target, no workspace, no atomics. */
int anirec_rows_rank(const float *scores, int64_t ld, int32_t n_anime, const uint32_t *watched, int32_t n_users,
                     const int32_t *target_row, const int32_t *target_anime, int32_t n_targets, int32_t *out_rank,
                     int32_t *err_flag, void *stream);

/* Item-kNN score rows from user histories and truncated neighbour lists.  nbr_idx / nbr_sim are [n_items][K] (what
 * anirec_cooc_scores + anirec_rows_topk give per item; index < 0 is padding); list l's history is the entries
 * e = hist_offsets[l] .. hist_offsets[l+1]-1 of hist_idx / hist_w (CSR over n_hist entries; hist_w NULL means 1.0f).
 * For entry e (i = hist_idx[e], weight w) and slot s with j = nbr_idx[i][s] >= 0:
 *   term = llrint((double)w * (double)nbr_sim[i][s] * 2^30)     (the product is exact, the rounding to nearest even)
 *   S[l][j] += term as int64;     out_scores[l][j] = (float)((double)S[l][j] * 2^-30)
 * Every element of every output row is written, 0 where nothing landed.  A repeated history item counts twice.  A
 * term needs w and sim finite and |w sim| <= 1024; the documented bound is history length x K < 2^22 per list.
 * *err_flag (device; overwritten by the call) becomes 1 on an unusable term, a history item outside [0, n_items) or a
 * neighbour index >= n_items (that term, entry or slot adds nothing) and on an offsets pair that is negative,
 * decreasing or past n_hist (that list's row is NaN); nothing is read through the bad value and the other lists are
 * unaffected.  A list's row depends on that list's multiset of entries and the neighbour tables alone: not on entry
 * order, the other lists or the launch shape.  Integer atomics only: in LDS when n_items <=
 * anirec_itemknn_lds_items(), else on the list's int64 row of ws.
 * n_items < 1, K < 1, a negative count, or a NULL nbr_idx, nbr_sim, hist_offsets, out_scores, err_flag or ws
 * (hist_idx with n_hist > 0) with n_lists > 0: ANIREC_EINVAL before anything is enqueued or written.  n_lists == 0:
 * ANIREC_OK.  ws: anirec_itemknn_workspace_bytes(n_items, n_lists) bytes (0 for a bad argument), 8-byte aligned, less
 * is ANIREC_EWORKSPACE; the result does not depend on what it held.  Graph-capturable. */
size_t anirec_itemknn_lds_items(void);
size_t anirec_itemknn_workspace_bytes(int32_t n_items, int32_t n_lists);
int anirec_itemknn_scores(const int32_t *nbr_idx, const float *nbr_sim, int32_t n_items, int32_t K,
                          const int32_t *hist_offsets, const int32_t *hist_idx, const float *hist_w, int32_t n_lists,
                          int32_t n_hist, float *out_scores, int32_t *err_flag, void *ws, size_t ws_bytes,
                          void *stream);

/* CONTENT-BASED SCORE ROWS from item metadata: the one system that scores an item nobody has rated.
 * The item features are a CSR over n_tokens token ids: row j is the entries t = tok_offsets[j] .. tok_offsets[j+1]-1 of
 * tok_idx / tok_w (TF-IDF weights; tok_offsets int64 [n_items + 1], ascending from 0 — it is trusted: the call is not
 * told the arrays' length).  The histories are the CSR anirec_itemknn_scores takes (hist_w NULL means 1.0f; a negative
 * weight pushes away from a title).  out_scores is [n_lists][n_items].  The rule, for list l with entries e (item
 * i_e = hist_idx[e], weight w_e):
 *   Wq   = sum_e llrint(|w_e| * 2^30)                                                            as int64
 *   P[v] = sum_e sum_{t in row(i_e), tok_idx[t] == v} llrint((double)w_e * (double)tok_w[t] * 2^30)   as int64
 *          (the product of two fp32 values is exact in fp64: each term has one rounding, to the nearest even integer;
 *          a repeated item or a repeated token adds again)
 *   p[v] = Wq > 0 ? (float)((double)P[v] / (double)Wq) : 0.0f
 *          (two correctly rounded int64 -> fp64 conversions, one correctly rounded divide, one rounding to fp32: the
 *          weighted mean item vector, so scores are on one scale across users)
 *   out[l][j] = acc after acc = fmaf(p[tok_idx[t]], tok_w[t], acc) over t = tok_offsets[j] .. tok_offsets[j+1]-1 in
 *          storage order, from +0.0f: an item without tokens scores +0.0f
 * Integer sums followed by a fixed chain: a list's row depends on that list's multiset of entries and the item CSR
 * alone, not on entry order, the other lists of the call or the launch shape.  The documented bound is (history length
 * x longest item row) < 2^22 per list.
 * *err_flag (device; overwritten by the call) becomes 1, and the offending part adds nothing, on: a history entry whose
 * item is outside [0, n_items) or whose weight is not finite or above 1024 in magnitude (the entry adds nothing, to Wq
 * either); a token slot whose id is outside [0, n_tokens) or whose weight is not finite (the slot is skipped in the
 * profile and in the chain); a profile term with |w x| > 1024.  An offsets pair that is negative, decreasing or past
 * n_hist raises it too and makes that list's row NaN; nothing is read through a bad value and the other lists are
 * unaffected.
 * One workgroup per list; the int64 profile, and its fp32 image in place, live in LDS when n_tokens <=
 * anirec_content_lds_tokens(); above it the profile is on the list's int64 row of ws, the image still in LDS up to
 * twice that many tokens and on the ws row beyond.
 * n_items < 1, n_tokens < 1, a negative count, or a NULL tok_offsets, tok_idx, tok_w, hist_offsets, out_scores,
 * err_flag or ws (hist_idx with n_hist > 0) with n_lists > 0: ANIREC_EINVAL before anything is enqueued or written.
 * n_lists == 0: ANIREC_OK.  ws: anirec_content_workspace_bytes(n_tokens, n_lists) bytes (0 for a bad argument), 8-byte
 * aligned, less is ANIREC_EWORKSPACE; the result does not depend on what it or out_scores held.  Graph-capturable. */
size_t anirec_content_lds_tokens(void);
size_t anirec_content_workspace_bytes(int32_t n_tokens, int32_t n_lists);
int anirec_content_scores(const int64_t *tok_offsets, const int32_t *tok_idx, const float *tok_w, int32_t n_items,
                          int32_t n_tokens, const int32_t *hist_offsets, const int32_t *hist_idx, const float *hist_w,
                          int32_t n_lists, int32_t n_hist, float *out_scores, int32_t *err_flag, void *ws,
                          size_t ws_bytes, void *stream);

/* ONBOARDING LISTS: which m items to show a newcomer so that there is something to fit.  A greedy
 * maximum-coverage questionnaire over the rated-by bit rows: pick the m items such that as many users of a population
 * as possible have rated at least `depth` of them.  item_bits is [n_items][W] uint32, W = ceil(n_users/32), exactly as
 * anirec_cooc_scores takes it; bits at positions >= n_users may hold anything and have no effect, in the rows and in
 * open_bits alike.
 *
 * anirec_cover_greedy, the rule:
 *   population P   user u < n_users is in P iff open_bits is NULL or bit u of open_bits[W] is set
 *   level          level_u = 0 for every u; user u is OPEN iff u is in P and level_u < depth
 *   pick p = 0 .. m-1:
 *     gain_p(i)    the number of open users whose bit is set in row i
 *     candidates   the items with keep[i] != 0 (every item when keep is NULL) that are not picked yet
 *     the pick     the candidate of the largest gain, ties to the lowest index
 *     stop         no candidate, or a largest gain of 0: out_pick[p .. m-1] = -1, out_gain[p .. m-1] = 0
 *     otherwise    out_pick[p] = i, out_gain[p] = gain_p(i), and level_u += 1 for every open u of row i
 *   out_info[4]    {picks made, #{u in P : level_u == depth} at the end, |P|, 0}
 * So sum(out_gain) = the sum over P of min(depth, picked rows holding u), out_gain never increases, and depth >= m
 * never closes a user: the list is then "most rated within P", ties by index — the popularity questionnaire from the
 * same call.  The objective is monotone and submodular, so greedy is within 1 - 1/e of the best list.  Every quantity
 * is an integer count: a list depends on the bits, open_bits, keep, depth and m alone, not on the launch shape, on what
 * ws held, or on the rows the gain pass does not read (those that are no candidate).
 * Per pick two plain launches, all m enqueued at once: a gain pass (a wave per row, anirec_cover_step_words() words per
 * step of its row loop, 16-byte loads from the row's first 16-byte boundary, one 64-bit atomicMax of the key
 * gain << 32 | 0xFFFFFFFF - index per workgroup; the open mask in LDS up to anirec_cover_lds_words() words, past that
 * read from global memory) and a tail (writes the pick, raises the levels — bit planes over the
 * mask's words — and closes users).  Once the stop rule fires the remaining gain launches return on a device word.  No
 * workgroup waits on another, no host read-back, no cooperative grid: graph-capturable.
 * n_items < 1, n_users < 1, depth < 1, m outside 1 .. ANIREC_COVER_MAX_PICKS, a NULL item_bits, out_pick, out_gain,
 * out_info or ws, or a ws not 16-byte aligned: ANIREC_EINVAL before anything is enqueued or written.  ws:
 * anirec_cover_workspace_bytes(n_items, n_users) bytes (0 for a bad argument), less is ANIREC_EWORKSPACE; it may hold
 * anything on entry.  Cost: a pick reads n_items * W * 4 bytes less the picked and unkept rows.
 *
 * anirec_cover_levels: out_level[u], u < n_users, = the number of entries t < n_picks with picks[t] in [0, n_items) and
 * bit u of that row set: any list scored against any users (held-out users, a hand-made questionnaire).  An entry -1 is
 * skipped silently, so out_pick can be fed straight back; any other entry out of range raises *err_flag (device;
 * overwritten by the call) and is skipped, nothing is read through it; a repeated entry counts twice.  n_picks == 0
 * writes zeros.  n_items < 1, n_users < 1, n_picks < 0, a NULL item_bits, out_level or err_flag, a NULL picks with
 * n_picks > 0: ANIREC_EINVAL before anything is enqueued or written.  No workspace.  Graph-capturable. */
#define ANIREC_COVER_MAX_PICKS 1024
size_t anirec_cover_step_words(void);
size_t anirec_cover_lds_words(void);
size_t anirec_cover_workspace_bytes(int32_t n_items, int32_t n_users);
int anirec_cover_greedy(const uint32_t *item_bits, int32_t n_items, int32_t n_users, const uint32_t *open_bits,
                        const uint8_t *keep, int32_t depth, int32_t m, int32_t *out_pick, int32_t *out_gain,
                        int32_t *out_info, void *ws, size_t ws_bytes, void *stream);
int anirec_cover_levels(const uint32_t *item_bits, int32_t n_items, int32_t n_users, const int32_t *picks,
                        int32_t n_picks, int32_t *out_level, int32_t *err_flag, void *stream);

/* ------------------------------------------------------------------------- *
 *  HYBRID LISTS: several systems' score rows fused into one.  Every system ends in fp32 score rows
 *  [nq][n] on a scale of its own, so the fusion is per row and scale-free: reciprocal rank fusion (Cormack, Clarke and
 *  Buettcher 2009) or CombSUM of min-max normalised scores (Fox and Shaw 1994), both under the row's own mask.
 *
 *  rows_host[s], s < n_sys, is a DEVICE pointer to system s's rows, ld_host[s] the floats between two of them (0: one
 *  vector shared by every row, as anirec_rows_rank has it); the two arrays and weight_host are HOST arrays, read
 *  before the call returns (they travel in the kernel's argument struct).  watched: optional [nq][ceil(n/32)] words, a
 *  set bit excludes (bits at positions >= n are ignored); keep: optional [n] bytes.  Item j of row t is ELIGIBLE when
 *  keep[j] != 0 and its watched bit is clear.  out[t * ld_out + j] is the fused value of an eligible j and the
 *  canonical NaN (0x7FC00000) of any other j < n; columns n .. ld_out are not written.  Nothing is read back: the call
 *  is stream-ordered and can be captured into a graph.
 *
 *  The order of a row is the select's: score_key descending (larger first, +0 above -0, NaN after every number), ties
 *  to the ascending index.  r_s(t, j) = the 0-based place of an eligible j among the eligible items of row t in
 *  system s.
 *    ANIREC_FUSE_RRF     term_s = fl32(w_s / fl32(rrf_c + 1 + r_s)): the integer is exact in fp32, the division is
 *                        correctly rounded.  NaN scores are eligible and rank last, by index.
 *    ANIREC_FUSE_MINMAX  hi / lo = the first / the last FINITE eligible score of the row in the order above (chosen by
 *                        key: a row holding both zeros has one answer); v_s = fl32(fl32(x - lo) / fl32(hi - lo)) for a
 *                        finite x, 0 where hi - lo == 0 or the row has no finite eligible score, 1 for +inf, 0 for
 *                        -inf and NaN; term_s = fl32(w_s * v_s).
 *  out = ((+0 + term_0) + term_1) + ... in system order, every add rounded, nothing contracted: a pure function of
 *  the row's values, equal to a NumPy restatement bit for bit.
 *
 *  ANIREC_EINVAL before any launch: n_sys outside 1 .. ANIREC_FUSE_MAX_SYS, n outside 1 .. anirec_fuse_max_items()
 *  (one row's sort image in LDS), nq < 0, an ld_host[s] that is neither 0 nor >= n, ld_out < n, an unknown method,
 *  rrf_c outside 0 .. 2^20, a weight that is negative or not finite, weights that are all zero, a null rows_host,
 *  ld_host, weight_host, rows_host[s] or out.  nq == 0: ANIREC_OK, nothing launched.
 * ------------------------------------------------------------------------- */
#define ANIREC_FUSE_RRF     0
#define ANIREC_FUSE_MINMAX  1
#define ANIREC_FUSE_MAX_SYS 8
size_t anirec_fuse_max_items(void);
int anirec_fuse_rows(const float *const *rows_host, const int64_t *ld_host, int32_t n_sys, int32_t n, int32_t nq,
                     const uint32_t *watched, const uint8_t *keep, const float *weight_host, int32_t method,
                     int32_t rrf_c, float *out, int64_t ld_out, void *stream);

/* anirec_fuse_rank_grid: the rank of every held-out target under every candidate weight vector, without a fused row
 * (DESIGN.md 4.22).  rows_host, ld_host, n_sys, n, watched, keep, method and rrf_c are anirec_fuse_rows' over n_rows
 * rows; weights is a DEVICE array [n_w][n_sys]; target t is (target_row[t]: a row, target_anime[t]: an item).  For every
 * w < n_w and t < n_targets
 *   out_rank[w * n_targets + t] = #{ eligible j of row target_row[t] :
 *                                    (score_key(fused_w(t, j)) << 32 | ~j)  >  (score_key(fused_w(t, a)) << 32 | ~a) },
 * a = target_anime[t], fused_w(t, j) the value anirec_fuse_rows writes at out[t][j] with weight_host = weights[w]: the
 * same fp32 steps (one correctly rounded division, or one product, per term; the adds in system order from +0; nothing
 * contracted).  That is exactly what anirec_rows_rank returns for the target on that fused row under the same watched
 * bits.  (With a keep, an item that is not kept holds NaN in the fused row, which anirec_rows_rank, knowing no keep,
 * would count above a target whose own fused value is NaN; the grid counts eligible items alone.)  The layout is the
 * ranks [n_sys][n_t] anirec_rank_gain_rows takes, one "system" per weight vector: hence ANIREC_FUSE_MAX_GRID, its
 * column bound with one metric.
 * A system's place in a row, and its min-max normalised score, do not depend on the weights: a first kernel (a
 * workgroup per row, anirec_fuse_rows' own sort or extrema) writes per row, system and item the int32 c + 1 + r_s or
 * the fp32 v_s to ws; a second (a workgroup per target and 64 weight vectors, a lane per vector) walks them and counts.
 * *err_flag (device; overwritten by the call) becomes 1, and the ranks named are -1, for a target_row outside
 * [0, n_rows), a target_anime outside [0, n), a target that is not eligible in its own row (out_rank[.][t]) and for a
 * weight vector that holds a negative, NaN or infinite entry or is all zero (out_rank[w][.]); nothing is read through a
 * bad index and the other targets and vectors are unaffected.
 * ANIREC_EINVAL before any launch: what anirec_fuse_rows refuses for the arguments both have, n_w outside
 * 1 .. ANIREC_FUSE_MAX_GRID, n_targets < 0, a NULL weights, out_rank or err_flag, a NULL target array with
 * n_targets > 0, a ws that is NULL or not 16-byte aligned.  ws: anirec_fuse_rank_grid_workspace_bytes(n_sys, n, n_rows,
 * method) bytes (0 for a bad argument; needs no GPU), less is ANIREC_EWORKSPACE; the result does not depend on what it
 * held.  n_targets == 0 or n_rows == 0: ANIREC_OK, nothing launched.  No float atomics, nothing read back:
 * stream-ordered and graph-capturable. */
#define ANIREC_FUSE_MAX_GRID 4095
size_t anirec_fuse_rank_grid_workspace_bytes(int32_t n_sys, int32_t n, int32_t n_rows, int32_t method);
int anirec_fuse_rank_grid(const float *const *rows_host, const int64_t *ld_host, int32_t n_sys, int32_t n,
                          int32_t n_rows, const uint32_t *watched, const uint8_t *keep, int32_t method, int32_t rrf_c,
                          const float *weights, int32_t n_w, const int32_t *target_row, const int32_t *target_anime,
                          int32_t n_targets, int32_t *out_rank, int32_t *err_flag, void *ws, size_t ws_bytes,
                          void *stream);

/* ------------------------------------------------------------------------- *
 *  IMPLICIT-FEEDBACK ALS (Hu, Koren, Volinsky 2008) with the warm-started conjugate-gradient solve of Takacs, Pilaszy
 *  and Tikk (2011): the learned baseline a ranking table is read against.  No model takes part.
 *  Tables X [n_users][dim], Y [n_items][dim], dim one of 32, 64, 128, 256.  A liked pair (u, i) carries a confidence
 *  excess e_ui >= 0 (confidence c = 1 + e) and preference 1; every other pair preference 0 and confidence 1.  The
 *  objective is sum_all c_ui (p_ui - x_u . y_i)^2 + lambda (|X|^2 + |Y|^2).  All arithmetic below is fp32 unless it
 *  says fp64; there are no float atomics and no kernel waits on another workgroup.
 *
 * anirec_als_gram: G_out [dim][dim] = Y^T Y for Y [n][dim].  Every product Y[r][a] * Y[r][b] is taken in fp64, where it
 * is exact; the rows are cut into chunks of ANIREC_ALS_GRAM_CHUNK, a cell's products are added in fp64 in row order
 * inside a chunk, the chunk partials in chunk order from chunk 0's, and the sum is rounded once to fp32.  So
 * |G - G64| <= 2^-24 |G64| + n 2^-52 sum_r |Y[r][a] Y[r][b]| for finite input, and the bits depend on Y and n alone.
 * n < 1, a bad dim, a NULL Y, G_out or workspace, a workspace not 8-byte aligned: ANIREC_EINVAL before anything is
 * enqueued.  workspace: anirec_als_gram_workspace_bytes(n, dim) bytes (0 for a bad argument; needs no GPU), less is
 * ANIREC_EWORKSPACE; the result does not depend on what it held.  Graph-capturable.
 *
 * anirec_als_half_sweep: refits every row of X_inout [n_rows][dim] in place with Y [n_other][dim] frozen and
 * G = Y^T Y (anirec_als_gram's, or any [dim][dim] the caller holds; only its rows are read, as a symmetric matrix's).
 * Row u's list I is the entries k = offsets[u] .. offsets[u+1]-1: item i_k = idx[k], excess e_k = excess[k], or alpha
 * for every entry when excess is NULL.  A repeated index is two entries.  With
 *     A v  :=  G v + lambda v + sum_{k in I} e_k (y_k . v) y_k                          (never formed as a matrix)
 * the row is
 *     empty list:  x = 0 exactly, row_loss = 0, no iteration
 *     cg_steps == 0:  x stays bit for bit
 *     r = sum_k ((1 + e_k) - e_k (y_k . x)) y_k - G x - lambda x;   p = r;   rs0 = rs = r . r
 *     for t = 1 .. cg_steps:   stop unless rs > ANIREC_ALS_CG_RTOL2 * rs0        (which also stops rs0 == 0 and NaN)
 *         a = rs / (p . Ap);  x += a p;  r -= a Ap;  rs' = r . r;  p = r + (rs' / rs) p;  rs = rs'
 *     row_loss = x . G x + sum_k [ (1 + e_k)(1 - s_k)^2 - s_k^2 ] + lambda x . x,   s_k = y_k . x, at the final x
 * (row_loss is the row's share of the objective over ALL items, the constant sum over the unlisted items of 0 dropped
 * into x . G x - sum_k s_k^2.)  The item half-sweep is the same call on the transposed CSR with X as the frozen table.
 * The order of every sum, nothing contracted into an fma (kNG = 1024 / dim lane groups, group g, lane l = 0 .. dim/4-1
 * holding elements 4l .. 4l+3):
 *     u . v     per lane ((u0 v0 + u1 v1) + u2 v2) + u3 v3, then the xor butterfly over the group's lanes at distances
 *               dim/8, dim/16, .., 1
 *     a walk    group g starts from 0, adds w_k G[k] for the rows k = g, g + kNG, .. of G (w_k = v[k]; -v[k] in r, where
 *               the list term follows in the same accumulator), then c_k y_k for the entries k = g, g + kNG, .. of the
 *               list in list order (c_k = e_k s_k in A v; (1 + e_k) - e_k s_k in r); the kNG partial rows are added in
 *               group order from group 0's; the lambda term is added (A v) or subtracted (r) last
 *     row_loss  (x . Gx + L) + lambda (x . x), L the groups' sums of ((1 + e_k) (d d) - s_k s_k), d = 1 - s_k, over
 *               their entries in list order, added in group order
 * So a row's bits are a function of its own list, its start row, Y, G and the scalars: the same alone or among any
 * other rows, at any position, under any `order`, from run to run.
 * order: NULL, or a permutation of 0 .. n_rows-1: workgroup b takes row order[b] (longest lists first keeps the tail
 * short).  A value outside [0, n_rows) raises *err_flag and fits nothing; a value that repeats is undefined.
 * *err_flag (device; overwritten by the call) becomes 1 on an index outside [0, n_other) or an offsets pair that is
 * negative, decreasing or longer than INT32_MAX: that row and its loss are NaN, nothing is read through the bad value,
 * the other rows are unaffected.  excess must be finite and >= 0 (the caller's check; the kernel takes what it is given).
 * A bad dim, n_other < 1, n_rows < 0, cg_steps outside 0 .. ANIREC_ALS_MAX_CG, lambda or alpha negative or not finite, a
 * NULL Y, G, offsets, X_inout, row_loss or err_flag with n_rows > 0: ANIREC_EINVAL before anything is enqueued.
 * n_rows == 0: ANIREC_OK.  No workspace.  Every loop is bounded by cg_steps and the list length.  Graph-capturable.
 *
 * anirec_dot_scores: out[q][j] = the chain acc = fmaf(Q[q][t], Y[j][t], acc), t = 0 .. dim-1, from 0, for Q [n_q][dim]
 * and Y [n][dim]; out is [n_q][ld], ld >= n, elements j >= n of a row are not written.  It is anirec_cosine_scores_w's
 * chain (the same kernels) on rows that need not be normalised: the score rows anirec_rows_topk / anirec_rows_rank
 * take.  n < 1, n_q outside 0 .. 4 194 240, ld < n, a bad dim or a NULL pointer with n_q > 0: ANIREC_EINVAL.
 * ------------------------------------------------------------------------- */
#define ANIREC_ALS_MAX_CG 16         /* the most conjugate-gradient steps of a half-sweep */
#define ANIREC_ALS_CG_RTOL2 1e-10f   /* a row stops iterating once r . r <= this x its first r . r */
#define ANIREC_ALS_GRAM_CHUNK 1024   /* rows of one chunk of anirec_als_gram: part of its definition, not a knob */
size_t anirec_als_gram_workspace_bytes(int32_t n, int32_t dim);
int anirec_als_gram(const float *Y, int32_t n, int32_t dim, float *G_out, void *workspace, size_t workspace_bytes,
                    void *stream);
int anirec_als_half_sweep(const float *Y, int32_t n_other, int32_t dim, const float *G, const int64_t *offsets,
                          const int32_t *idx, const float *excess, float alpha, const int32_t *order, float *X_inout,
                          int32_t n_rows, float lambda, int32_t cg_steps, float *row_loss, int32_t *err_flag,
                          void *stream);
int anirec_dot_scores(const float *Q, int32_t n_q, const float *Y, int32_t n, int32_t dim, float *out, int64_t ld,
                      void *stream);

/* ------------------------------------------------------------------------- *
 *  BPR MATRIX FACTORISATION (Rendle, Freudenthaler, Gantner and Schmidt-Thieme 2009, "BPR: Bayesian Personalized Ranking
 *  from Implicit Feedback"): the learned baseline with a PAIRWISE objective.  No model takes part.
 *  Mini-batch SGD ascent on sum ln sigmoid(x_u . (y_i - y_j)) - reg (|x_u|^2 + |y_i|^2 + |y_j|^2) / 2 over sampled
 *  triples (u, liked i, unliked j).  Every quantity that crosses a slot is an integer, so the result is a function of
 *  the inputs alone: not of the launch shape, the order of the atomics or the run.
 *
 * Inputs.  The distinct liked pairs as a CSR by user: offsets int64 [n_users + 1], idx int32 [nnz], the items ascending
 * inside a row without repeats (the caller's promise; the binary search below needs it), and pair_user int32 [nnz], the
 * row of every entry.  1 <= nnz < 2^31.  Tables X [n_users][width], Y [n_items][width], fp32, 16-byte aligned, width one
 * of 32, 64, 128, 256, updated in place.
 *
 * Draws, all in uint32 arithmetic mod 2^32, mix32 as in the bootstrap section above:
 *     h(t, s)    = mix32( mix32(seed + 0x9e3779b9 * t) ^ mix32(s + 0x85ebca6b) )
 *     r(t, s, c) = mix32( h(t, s) + 0x9e3779b9 * (c + 1) )
 *     pick(r, n) = (uint64(r) * n) >> 32
 * Step t, slot s < batch: the positive pair is p = pick(r(t, s, 0), nnz), u = pair_user[p], i = idx[p]; the negative is
 * the first j = pick(r(t, s, c), n_items), c = 1 .. tries, that is not in u's row (binary search).  If all `tries`
 * candidates are liked the slot is DROPPED: it contributes nothing.  1 <= tries <= ANIREC_BPR_MAX_TRIES.
 *
 * Gradient of step t, every slot against the tables as they stand BEFORE the step; fp32, nothing contracted:
 *     d[k] = y_i[k] - y_j[k]
 *     x^   = sum_k x_u[k] d[k]: lane l = 0 .. width/4-1 holds elements 4l .. 4l+3 and takes
 *            ((x0 d0 + x1 d1) + x2 d2) + x3 d3; then the xor butterfly v[l] += v[l ^ o] over the lanes at distances
 *            o = width/8, width/16, .., 1 (anirec_als_half_sweep's u . v)
 *     g    = 1 / (1 + e(x^)), with e(x) operation by operation:
 *            xc = fmin(fmax(x, -30), 30)   (a NaN becomes -30);   kf = rint(xc * L2E)   (to nearest, ties to even)
 *            r = (xc - kf * C1) - kf * C2;   p = ((((((P6 r + P5) r + P4) r + P3) r + P2) r + 1) r + 1   (Horner)
 *            e = ldexp(p, kf);   g = 1 / (1 + e)   (one IEEE divide)
 *            L2E = 0x3FB8AA3B, C1 = 0x3F317200, C2 = 0x35BFBE8E (ln 2 = C1 + C2), P6 .. P2 = fp32(1/720), fp32(1/120),
 *            fp32(1/24), fp32(1/6), 0.5.  No expf: a NumPy restatement gives g bit for bit.  |g - logistic(-x^)| < 1e-6.
 *     terms: row u gets llrint((double)(float)(g * d[k]) * 2^30) in column k; row i gets
 *            llrint((double)(float)(g * x_u[k]) * 2^30), row j its negative.  A product that is not finite or above 2^20
 *            in magnitude contributes 0 and sets ANIREC_BPR_ERR_DIVERGED in *err_flag.
 * The terms are summed as int64 (mod 2^64) per (row, column), and every row counts the slots that touch it (c).
 * Update, every row with c > 0, plain fp32 operations in this order:
 *     grad = (float)((double)sum * 2^-30);    x <- x + lr * (grad - (reg * (float)c) * x)
 * With bias = 1 column width-1 of the USER rows is never written: the caller sets it to 1 (and the items' column to 0 at
 * the start), which makes the items' column width-1 an item bias while the scores stay anirec_dot_scores'.
 * out_counts [n_steps][3] int64: per step the slots kept, the slots dropped and the kept slots with x^ > 0.
 *
 * anirec_bpr_steps runs the steps step0 .. step0 + n_steps - 1 in place; all launches are enqueued at once, nothing is
 * read back: graph-capturable.  A step is two launches: the gradient phase reads the tables and writes accumulators
 * only; the apply phase writes the tables, each touched row once, and scans no table.
 * workspace: anirec_bpr_workspace_bytes(n_users, n_items, width, batch) bytes (0 for a bad argument; needs no GPU), less
 * is ANIREC_EWORKSPACE; the call zeroes what it uses, so the result does not depend on what the workspace held.
 * *err_flag (device; overwritten by the call): ANIREC_BPR_ERR_INDEX on a pair_user or idx entry out of range at a drawn
 * pair, or an offsets pair of the drawn user that is negative, decreasing or past nnz: nothing is read through the bad
 * value and the slot counts as dropped; ANIREC_BPR_ERR_DIVERGED as above.
 * A bad width, n_users or n_items < 1, nnz outside 1 .. 2^31-1, batch < 1, tries outside 1 .. ANIREC_BPR_MAX_TRIES,
 * step0 < 0, n_steps < 0, step0 + n_steps > INT32_MAX, lr or reg negative or not finite, bias not 0 or 1, a NULL pointer
 * (out_counts may be NULL with n_steps == 0), tables not 16-byte or workspace / out_counts not 8-byte aligned:
 * ANIREC_EINVAL before anything is enqueued.  n_steps == 0: ANIREC_OK, the tables untouched.
 *
 * anirec_bpr_sample: out_triples int32 [n_steps][batch][3] = (u, i, j) of the steps step0 .. step0 + n_steps - 1 as
 * anirec_bpr_steps draws them; j = -1 for a dropped slot, (-1, -1, -1) and ANIREC_BPR_ERR_INDEX for an index out of
 * range.  The same argument rules.
 * ------------------------------------------------------------------------- */
#define ANIREC_BPR_MAX_TRIES 16     /* the most negative candidates of a slot */
#define ANIREC_BPR_ERR_INDEX 1      /* *err_flag bit: an index out of range */
#define ANIREC_BPR_ERR_DIVERGED 2   /* *err_flag bit: a gradient term not finite or above 2^20 */
size_t anirec_bpr_workspace_bytes(int32_t n_users, int32_t n_items, int32_t width, int32_t batch);
int anirec_bpr_sample(const int64_t *offsets, const int32_t *idx, const int32_t *pair_user, int32_t n_users,
                      int32_t n_items, int64_t nnz, int32_t batch, int32_t tries, uint32_t seed, int32_t step0,
                      int32_t n_steps, int32_t *out_triples, int32_t *err_flag, void *stream);
int anirec_bpr_steps(float *X, float *Y, int32_t n_users, int32_t n_items, int32_t width, const int64_t *offsets,
                     const int32_t *idx, const int32_t *pair_user, int64_t nnz, int32_t batch, int32_t tries,
                     uint32_t seed, int32_t step0, int32_t n_steps, float lr, float reg, int32_t bias,
                     int64_t *out_counts, int32_t *err_flag, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------- *
 *  EASE (Steck 2019, "Embarrassingly Shallow Autoencoders for Sparse Data"): the linear item-item autoencoder a
 *  ranking table reads item-kNN and ALS against.  With B the n_items x n_users 0/1 matrix of liked
 *  pairs: G = B B^T (anirec_cooc_scores' out_count rows), A = G + reg I, P = A^-1, W[i][j] = -P[i][j] / P[j][j] off the
 *  diagonal and 0 on it; a history H scores item j as sum_{i in H} w_i W[i][j].  Every call below is stream-ordered
 *  plain launches: no host read-back, no cooperative launch, no float atomics, no kernel that waits on another
 *  workgroup, every loop bounded by the arguments.  Graph-capturable.  All indexing is 64-bit.
 *
 * anirec_spd_inverse: A_inout [n][ld] fp64, symmetric positive definite, is replaced by its inverse (elements j >= n of
 * a row are neither read nor written).  The route is part of the definition: blocked Gauss-Jordan elimination in
 * place, without pivoting, NB = anirec_spd_inverse_block() (a constant, not a knob), T = ceil(n / NB) block steps.
 * Block step b, K = the rows b NB .. min(n, (b + 1) NB) - 1, every block padded to NB x NB (the diagonal block with the
 * identity, any other with zeros):
 *     R  = A[K][K]^-1, by the unblocked form of the same elimination: for p = 0 .. NB-1 in order, t = 1 / D[p][p],
 *          row[j] = D[p][j] t, col[i] = D[i][p];  D[i][j] = fma(-col[i], row[j], D[i][j]) for i, j != p;
 *          D[p][j] = row[j];  D[i][p] = -(col[i] t);  D[p][p] = t
 *     Rp = R A[K][:]   (NB x n; each element an fma chain over k = 0 .. NB-1 from 0), with Rp[:][K] = R
 *     A[I][J] = A[I][J] - A[I][K] Rp[:][J]   for I, J outside K
 *     A[K][J] = Rp[:][J];   A[I][K] = -A[I][K] R;   A[K][K] = R
 *   the two products with A[I][K] summed over k ascending on v_mfma_f64_16x16x4_f64 (four k to an instruction), each
 *   output element by one lane.  The hardware's order inside one instruction is not documented, so the result is held
 *   to a residual, not to NumPy's bits: max |A P - I| <= 8 max(the same of a LAPACK inverse, n 2^-52) on the tested
 *   domain (co-occurrence counts with reg >= 1; a reg far below 1 on a rank-deficient G is outside it).
 *   The bits of the result are a function of A, n and ld alone: the same from run to run and whatever ws held.
 *   *info (device; overwritten by the call): 0 on success, else 1 + the first block step that met a pivot D[p][p] that
 *   was not > 0 or not finite; the call still runs every step in bounded time, reads nothing out of bounds, and leaves
 *   A_inout unspecified.
 *   n < 1, ld < n, n > 65535 NB, a NULL A_inout, info or ws, an A_inout or ws not 8-byte aligned, an info not 4-byte
 *   aligned: ANIREC_EINVAL before anything is enqueued.  ws: anirec_spd_inverse_workspace_bytes(n) bytes (0 for
 *   n < 1; needs no GPU), less is ANIREC_EWORKSPACE.
 *
 * anirec_ease_weights: W_out[i][j] = (float)(-P[i][j] / P[j][j]) for i != j (one correctly rounded fp64 divide, one
 * rounding to fp32), W_out[i][i] = +0.0f; P [n][ldp] fp64, W_out [n][ldw] fp32, elements j >= n of a row are not
 * written.  n < 1, ldp < n, ldw < n, a NULL or misaligned pointer: ANIREC_EINVAL.
 *
 * anirec_ease_scores: score rows from histories.  W [n_items][ldw]; the histories are the CSR anirec_itemknn_scores
 * takes (hist_w NULL means 1.0f) and the term rule is that call's, so the two agree bit for bit where they overlap:
 *     term = llrint((double)w * (double)W[i][j] * 2^30);  S[l][j] += term as int64;
 *     out_scores[l][j] = (float)((double)S[l][j] * 2^-30)          out_scores is [n_lists][ld]
 * Every element j < n_items of every row is written (0 for an empty list); elements past n_items are not.  A repeated
 * item counts twice.  A term needs w and W[i][j] finite and |w W[i][j]| <= 1024; the documented bound is 2^22 entries a
 * list.  A row depends on its list's multiset of entries and on W alone: not on entry order, the other lists or the
 * launch shape.  One thread owns an output element: no atomics, no workspace; the column tile
 * (anirec_ease_scores_col_tile() columns) is the slow grid index, a list's entries are staged
 * anirec_ease_scores_entry_tile() at a time.
 * *err_flag (device; overwritten by the call) becomes 1 on an unusable term or a history item outside [0, n_items)
 * (that term or entry adds nothing) and on an offsets pair that is negative, decreasing or past n_hist (that list's
 * row is NaN); nothing is read through the bad value and the other lists are unaffected.
 * n_items < 1, a negative count, ldw < n_items, ld < n_items, or a NULL W, hist_offsets, out_scores or err_flag
 * (hist_idx with n_hist > 0) with n_lists > 0: ANIREC_EINVAL before anything is enqueued.  n_lists == 0: ANIREC_OK.
 * ------------------------------------------------------------------------- */
int32_t anirec_spd_inverse_block(void);
size_t anirec_spd_inverse_workspace_bytes(int32_t n);
int anirec_spd_inverse(double *A_inout, int64_t ld, int32_t n, int32_t *info, void *ws, size_t ws_bytes,
                       void *stream);
int anirec_ease_weights(const double *P, int64_t ldp, int32_t n, float *W_out, int64_t ldw, void *stream);
int32_t anirec_ease_scores_col_tile(void);
int32_t anirec_ease_scores_entry_tile(void);
int anirec_ease_scores(const float *W, int64_t ldw, int32_t n_items, const int32_t *hist_offsets,
                       const int32_t *hist_idx, const float *hist_w, int32_t n_lists, int32_t n_hist,
                       float *out_scores, int64_t ld, int32_t *err_flag, void *stream);

/* ------------------------------------------------------------------------- *
 *  USER-WEIGHTED CO-OCCURRENCE on the i8 matrix cores: what the graph baselines P3alpha (Cooper et al. 2014) and
 *  RP3beta (Paudel et al. 2017) are built from.  item_bits as anirec_cooc_scores takes it; user_q
 *  [n_users] is an integer weight per user, 0 .. ANIREC_WCOOC_MAX_Q (14 bits: two 7-bit limbs of the signed i8
 *  operand).
 *
 * anirec_wcooc_scores: one row per query item q = queries[t], against every item j:
 *   S(q,j)   the sum of user_q[u] over the users u < n_users set in both row q and row j, exact in int64
 *   w        S != 0 ? (float)(((double)S * rs) * cs) : +0.0f, with rs = row_scale ? row_scale[q] : 1.0 and
 *            cs = col_scale ? col_scale[j] : 1.0; the two fp64 multiplies are rounded one by one, nothing contracted
 *   out_w [nq][n_items] = w; out_sum (optional) [nq][n_items] = S;
 *   out_excl (optional) [nq][ceil(n_items/32)]: bit j of row t set iff S == 0 or j == q — the mask rows
 *   anirec_rows_topk takes as wbits; bits at positions >= n_items are clear.
 * A query outside [0, n_items) raises *err_flag (device; overwritten by the call) to 1: its rows are NaN / -1 / every
 * bit j < n_items set, nothing is read through it, the other queries are unaffected.  A user_q outside its range counts
 * as 0 and raises the flag too.  A query may repeat.  A query's rows depend on that query, the bits, user_q and the two
 * scales alone: not on nq, its position in `queries`, the launch shape or what the workspace held.  Each limb is
 * accumulated in int32 by v_mfma_i32_16x16x64_i8: 127 * 2^24 < 2^31, so n_users <= 2^24 keeps every accumulator
 * exact and the call bit-reproducible.  A 256-thread workgroup owns 64 queries x 64 keys and stages
 * anirec_wcooc_chunk_words() user words of both row sets, and the limb bytes of those users, in LDS per pass.
 * n_items < 1, n_users outside 1 .. 2^24, a negative nq, or with nq > 0 a NULL item_bits, user_q, queries, out_w,
 * err_flag or ws, a pointer not aligned to its element (ws: 16 bytes): ANIREC_EINVAL before anything is enqueued or
 * written.  nq == 0: ANIREC_OK, nothing enqueued.  ws: anirec_wcooc_workspace_bytes(n_items, n_users, nq) bytes (0 for
 * a bad argument; the two limb byte arrays), less is ANIREC_EWORKSPACE.  Stream-ordered plain launches, no host
 * read-back: graph-capturable.
 * ------------------------------------------------------------------------- */
#define ANIREC_WCOOC_MAX_Q 16383
size_t anirec_wcooc_chunk_words(void);
size_t anirec_wcooc_workspace_bytes(int32_t n_items, int32_t n_users, int32_t nq);
int anirec_wcooc_scores(const uint32_t *item_bits, int32_t n_items, int32_t n_users, const int32_t *user_q,
                        const int32_t *queries, int32_t nq, const double *row_scale, const double *col_scale,
                        float *out_w, int64_t *out_sum, uint32_t *out_excl, int32_t *err_flag, void *ws,
                        size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------------- *
 *  Ranks to metric sums, and a Poisson bootstrap over users on them.  Integer sums throughout: no
 *  result depends on the order the rows are met in.
 *  The statistic: the resampling UNIT is the user (a user's held-out ratings are not independent, so a replicate
 *  re-weights whole users); replicate b >= 1 gives unit u an integer weight w(b, u), independent over (b, u) and
 *  Poisson(1) under the Poisson threshold table, drawn from a counter-based hash and never stored; replicate 0 is the
 *  sample itself (all weights 1).  A metric is a mean over targets of a gain that depends on the target's rank alone,
 *  held as a uint32 fixed-point table over ranks (rint(gain * 2^30); the mean rank: the rank at scale 1); replicate b's
 *  figure is sum_b[column] / (scale * sum_b[count]) in fp64 on the host.
 *
 * anirec_rank_gain_rows: ranks int32 [n_sys][n_t] (system s ranks target t at ranks[s][t]), target_unit int32 [n_t]
 * (the target's position in the unit list), gain uint32 [n_metric][n_gain] (a metric's fixed-point gain per rank).
 * out int64 [n_units][n_sys * n_metric + 1]: column s * n_metric + m is the sum over the unit's targets of
 * gain[m][ranks[s][t]], a rank < 0 or >= n_gain gaining 0 (a missed list slot's -1 needs no special case); the last
 * column is the unit's number of targets.  The call zeroes out itself.  *err_flag (device; overwritten) becomes 1 for
 * a target_unit outside [0, n_units): that target is dropped, nothing is read or written through it, the others are
 * unaffected.  A thread adds up a run of consecutive targets of one unit before it issues an atomic, so a unit with
 * many targets does not serialise the call.  n_sys, n_metric or n_gain < 1, a negative count, n_sys * n_metric + 1 >
 * 4096, a NULL err_flag, a NULL or misaligned (8 bytes) out with n_units > 0, or a NULL ranks, target_unit or gain
 * with n_t > 0: ANIREC_EINVAL before anything is enqueued or written.  Graph-capturable.
 *
 * anirec_boot_sums: values int64 [n_units][n_col] (anirec_rank_gain_rows' out, or any non-negative sums), unit_key
 * int32 [n_units].  out int64 [n_rep + 1][n_col]: out[b][c] = sum over u of w(b, unit_key[u]) * values[u][c], with
 *     mix32(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16      (uint32, mod 2^32)
 *     r = mix32( mix32(seed + 0x9e3779b9 * b) ^ mix32((uint32_t)key + 0x85ebca6b) )
 *     w(b, key) = #{ j < n_thr : r >= thr[j] }  for b >= 1;   w(0, key) = 1      (row 0 is the plain column sums)
 * thr: a HOST table of n_thr <= 16 ascending uint32, passed to the kernel by value (floor(2^32 CDF(j)) of a
 * distribution on 0, 1, 2, ... draws from it; n_thr == 0 gives all-zero weights).  The weight depends on the key, not
 * on the unit's position: a subset of the units gets the same weights in a call of its own, so the sums of two calls
 * over a split of the units add up to the whole call's, bit for bit.  Exactness guard: limit = 2^62 / (max(n_thr, 1) *
 * n_units); a value < 0 or >= limit sets *err_flag (device; overwritten) and every element of out is -1, so nothing
 * overflows silently.  n_units == 0 writes zeros.  ws: anirec_boot_workspace_bytes(n_units, n_col, n_rep) bytes (0 for a
 * bad argument; the unit splits' partial rows), 8-byte aligned, less is ANIREC_EWORKSPACE; the result does not depend
 * on what it held.  One lane is one replicate; a workgroup stages anirec_boot_tile() units in LDS and keeps
 * anirec_boot_col_tile(n_col) column sums per lane in registers, wider inputs go over a grid dimension.
 * n_units < 0, n_col outside 1 .. 4096, n_rep outside 0 .. 65536, n_thr outside 0 .. 16, a thr that decreases, a NULL
 * out or err_flag, a NULL values, unit_key or ws with n_units > 0, values, out or ws not 8-byte aligned: ANIREC_EINVAL
 * before anything is enqueued or written.  No atomics; graph-capturable.
 *
 * anirec_boot_weights: the weights themselves, out uint8 [n_rep][n_units], row b - 1 = replicate b = 1 .. n_rep, for
 * figures that are no sums (a median, a coverage) and for small cases.  The same argument rules. */
size_t anirec_boot_tile(void);
size_t anirec_boot_col_tile(int32_t n_col);
size_t anirec_boot_workspace_bytes(int32_t n_units, int32_t n_col, int32_t n_rep);
int anirec_rank_gain_rows(const int32_t *ranks, int32_t n_sys, int32_t n_t, const int32_t *target_unit, int32_t n_units,
                          const uint32_t *gain, int32_t n_metric, int32_t n_gain, int64_t *out, int32_t *err_flag,
                          void *stream);
int anirec_boot_sums(const int64_t *values, const int32_t *unit_key, int32_t n_units, int32_t n_col, uint32_t seed,
                     int32_t n_rep, const uint32_t *thr, int32_t n_thr, int64_t *out, int32_t *err_flag, void *ws,
                     size_t ws_bytes, void *stream);
int anirec_boot_weights(const int32_t *unit_key, int32_t n_units, uint32_t seed, int32_t n_rep, const uint32_t *thr,
                        int32_t n_thr, uint8_t *out, void *stream);

/* The same top-k on the matrix cores (the batched model_recs path: 100 k users x 18 k anime):
 * fp16 MFMA cosine candidates with a rigorous error window, the watched mask applied when a
 * candidate is appended, exact fp32 re-rank through the head.  Same results as
 * anirec_predict_topk; flags[n_users] (device) is non-zero for the rare user whose window could
 * not be proven complete (saturated head, > 256 survivors, fewer than k unwatched anime): its row
 * is -1/NaN and the caller re-runs it through anirec_predict_topk.  k <= ANIREC_MAX_TOPK - 1. */
size_t anirec_predict_topk_mfma_workspace_bytes(int32_t n_anime, int32_t n_users);
int anirec_predict_topk_mfma(const float *U, const float *A, int32_t n_anime, const int32_t *users,
                             int32_t n_users, const anirec_head *head_host, const uint32_t *watched,
                             int32_t k, int32_t *out_idx, float *out_p, int32_t *flags, void *workspace,
                             size_t workspace_bytes, void *stream);
/* Any activation: the ratings are non-decreasing in sign * cosine, so the same proof holds; a row whose k-th survivor
 * does not lie STRICTLY above the best rating a non-survivor could reach (flat regions: relu at y <= 0, softplus
 * underflowing to 0, saturated sigmoid / tanh) is flagged and falls back to the exact path. */
int anirec_predict_topk_mfma_act(const float *U, const float *A, int32_t n_anime, const int32_t *users,
                                 int32_t n_users, const anirec_head *head_host, int32_t activation,
                                 const uint32_t *watched, int32_t k, int32_t *out_idx, float *out_p, int32_t *flags,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------- *
 *  INGEST — the step before the hot path, columns resident in HBM.
 *  Replaces preprocess/preprocess.py:13-40 (drop_useless: drop_duplicates keep-first, dropna,
 *  watched/plan filters, users with < num_reviews ratings), :52-105 (drop_half_watched),
 *  :108-117 (scale_ratings, float64) and the id -> Series.unique() position encoding of
 *  neural_network/neural_network.py:41-60.  Surviving rows keep their order; results are
 *  bit-identical to pandas.
 * ------------------------------------------------------------------------- */
#define ANIREC_NULL_I32 INT32_MIN /* missing value of an integer column (pandas NaN) */

typedef struct anirec_ingest_opts {
  int32_t num_reviews;       /* keep users with at least this many surviving ratings */
  int32_t drop_unwatched;    /* drop rows with watched_episodes == 0 */
  int32_t drop_plan;         /* drop rows with watching_status == 6 */
  int32_t drop_half_watched; /* drop rows with watched < half of the anime's max watched */
  int32_t user_id_bound;     /* ids must lie in [0, bound): sizes of the direct-index tables */
  int32_t anime_id_bound;
} anirec_ingest_opts;

/* rating: float64, NaN = missing.  Outputs hold up to n rows; *n_out (device) receives the row
 * count; *err_flag (device) becomes 1 if a non-missing id is outside its bound (that row is
 * dropped).  1 <= n < 2^30.  The five input columns and the workspace must be 16-byte aligned
 * (ANIREC_EINVAL otherwise: the kernels read four rows per lane).  Any row order is accepted; a table
 * grouped by user (the raw animelist) finds its duplicate rows in LDS, chunk by chunk. */
/* Largest user_id and anime_id of the two columns (ANIREC_NULL_I32 if a column holds nothing else) in one pass:
 * out_max2[0] + 1 / out_max2[1] + 1 are the id bounds anirec_ingest_opts asks for.  Device pointers, 16-byte aligned
 * columns, stream-ordered. */
int anirec_ingest_id_max(const int32_t *user_id, const int32_t *anime_id, int64_t n, int32_t *out_max2, void *stream);
size_t anirec_ingest_workspace_bytes(int64_t n, int32_t user_id_bound, int32_t anime_id_bound);
int anirec_ingest_preprocess(const int32_t *user_id, const int32_t *anime_id, const double *rating,
                             const int32_t *watching_status, const int32_t *watched_episodes, int64_t n,
                             const anirec_ingest_opts *opts, int32_t *out_user_id, int32_t *out_anime_id,
                             double *out_rating, int32_t *out_status, int32_t *out_episodes, int64_t *n_out,
                             int32_t *err_flag, void *workspace, size_t workspace_bytes, void *stream);

/* With opts->drop_half_watched the reference's frame keeps two extra columns (preprocess.py:99-100,104):
 * max_eps = the anime's largest watched_episodes over the rows that survived drop_useless, and
 * half_eps = max_eps == 1 ? 1 : max_eps * .5.  Call right after anirec_ingest_preprocess with the SAME
 * n, opts and workspace (the per-anime maxima are still in it); rows [0, *n_out) are written. */
int anirec_ingest_half_columns(const int32_t *out_anime_id, const int64_t *n_out, int64_t n,
                               const anirec_ingest_opts *opts, int32_t *out_max_eps, double *out_half_eps,
                               const void *workspace, size_t workspace_bytes, void *stream);

/* out_index[i] = position of id[i] in the order of first appearance (pandas Series.unique());
 * out_uniques[j] = the j-th distinct id; *n_unique (device) = number of distinct ids.
 * id, out_index and the workspace must be 16-byte aligned. */
size_t anirec_ingest_encode_workspace_bytes(int64_t n, int32_t id_bound);
int anirec_ingest_encode(const int32_t *id, int64_t n, int32_t id_bound, int32_t *out_index,
                         int32_t *out_uniques, int64_t *n_unique, int32_t *err_flag, void *workspace,
                         size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------- *
 *  FAVOURITES + USER-BASED RECS — the consumer of the similar-users top-k.
 *  user_recs/user_recs.py:377-404 (fave_genres: a user's favourites are the anime rated at or above
 *  the 80th percentile of their own ratings, np.percentile 'linear', float64; also
 *  similar_users.py:203-256 get_fave_anime) and :708-760 (similar_user_recs: per query user, count how
 *  many of its similar users hold each anime as a favourite, drop the query's own favourites, rank).
 * ------------------------------------------------------------------------- */

/* fav_bits[n_users][ceil(n_anime/32)]: bit a of row u set iff rating(u, a) >= threshold[u];
 * threshold[u] = np.percentile(ratings of u, percentile) bit for bit (NaN for users without ratings).
 * Ratings must not contain NaN.  *err_flag (device) becomes 1 on an out-of-range index.
 * The three columns and the workspace must be 16-byte aligned (ANIREC_EINVAL otherwise).  A table grouped by user
 * (non-decreasing user_idx: the raw / preprocessed order) is detected on the device and takes the fast path: no CSR
 * copy, the bit rows built per user and written once. */
size_t anirec_fav_workspace_bytes(int64_t n_ratings, int32_t n_users);
int anirec_user_favourites(const int32_t *user_idx, const int32_t *anime_idx, const double *rating, int64_t n,
                           int32_t n_users, int32_t n_anime, double percentile, uint32_t *fav_bits,
                           double *threshold, int32_t *err_flag, void *workspace, size_t workspace_bytes,
                           void *stream);

/* sim_users[nq][k_sim]: similar users of query_users[q], best first, -1 = empty (k_sim <= 63, n_recs <= 256).
 * out_anime/out_count[nq][n_recs]: anime by (count desc, best similar-user rank asc, anime index asc),
 * -1 / 0 padded; anime that are favourites of the query user are skipped.  n_anime < 131072. */
int anirec_user_recs(const uint32_t *fav_bits, int32_t n_users, int32_t n_anime, const int32_t *query_users,
                     const int32_t *sim_users, int32_t nq, int32_t k_sim, int32_t n_recs, int32_t *out_anime,
                     int32_t *out_count, void *stream);

/* As anirec_user_recs, but the skipped set of query q is exclude_bits[q][ceil(n_anime/32)] (not the favourite row of a
 * query user), and when keep_bits != NULL only anime a with bit a of keep_bits[ceil(n_anime/32)] set are counted or
 * returned (user_recs.py:743,753: the reference skips the anime NAMED in the user_prefs CSV, and loses anime missing
 * from all_anime.csv).  Same limits and tie order as anirec_user_recs. */
int anirec_user_recs_ex(const uint32_t *fav_bits, int32_t n_users, int32_t n_anime, const int32_t *sim_users,
                        int32_t nq, int32_t k_sim, const uint32_t *exclude_bits, const uint32_t *keep_bits,
                        int32_t n_recs, int32_t *out_anime, int32_t *out_count, void *stream);

/* Favourite profiles (user_prefs.py:95-136 get_genres / get_sources over a user's favourites):
 * counts[r][c] = #{ a : bit a of fav_bits[users[r]] set and bit c of cat_bits[a] set }
 * users == NULL: r runs over every user 0..n_users-1 (n_rows == n_users).
 * cat_bits[n_anime][cat_words], cat_words = ceil(n_cat/32), 1 <= n_cat <= 128.
 * *err_flag (device) becomes 1 on a user index out of range; that row's counts are 0. */
int anirec_fave_profile(const uint32_t *fav_bits, int32_t n_users, int32_t n_anime, const int32_t *users,
                        int32_t n_rows, const uint32_t *cat_bits, int32_t n_cat, int32_t *counts, int32_t *err_flag,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ANIREC_H */
