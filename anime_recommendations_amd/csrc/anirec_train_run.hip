// The host loop of libanirec's training path: what a descriptor must satisfy, the block scheduler (run_blocks, Walk,
// train_step), the per-stage C entry points and size queries, the one-GPU trainer handle, and the multi-GPU stepper
// with its run-time RCCL binding.  Host code only: every kernel is launched by the unit that defines it, through the
// launch_* functions of anirec_train.hpp.  (The stepper and the trainer share run_blocks, a template over the step they
// enqueue, and set_metrics: one file holds both rather than a header that would carry the scheduler into every unit.)
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <rccl/rccl.h>  // types and prototypes only: the library is bound at run time (dlopen), never linked
#include <string.h>

#include <new>

#include "anirec_train.hpp"

namespace anirec {

// the update rule: a known kind, and the lazy update (Adam's only) not asked for with another; a known head
int check_opt(const anirec_train_desc *d) {
  if (!loss_ok(d->loss) || !act_ok(d->activation)) return ANIREC_EINVAL;
  if (d->optimizer < ANIREC_OPT_ADAM || d->optimizer > ANIREC_OPT_ADAGRAD) return ANIREC_EINVAL;
  if (d->lazy != 0 && d->optimizer != ANIREC_OPT_ADAM) return ANIREC_EINVAL;
  return ANIREC_OK;
}

// dim: the row width of the tables (the *_w entry points; ANIREC_DIM otherwise).  Another width than ANIREC_DIM runs the
// dense one-GPU step only
int check_desc(const anirec_train_desc *d, int dim) {
  if (!dim_ok(dim)) return ANIREC_EINVAL;
  if (!d || !d->W || !d->M || !d->V || !d->rowmap || !d->state || !d->workspace || !d->packets)
    return ANIREC_EINVAL;
  if (dim != kDim && (d->lazy != 0 || d->dense_mode != 0 || d->n_seg != 1)) return ANIREC_EINVAL;
  if (d->max_batch < 1 || d->max_batch > ANIREC_MAX_BATCH) return ANIREC_EINVAL;
  if (d->n_user_rows < 1 || d->n_anime_rows < 1 || d->arena_steps < 2) return ANIREC_EINVAL;
  if (d->n_seg < 1 || d->n_seg > ANIREC_MAX_SEG || d->my_seg < 0 || d->my_seg >= d->n_seg)
    return ANIREC_EINVAL;
  if (d->dense_mode < 0 || d->dense_mode > 2) return ANIREC_EINVAL;
  if (check_opt(d)) return ANIREC_EINVAL;
  if (d->dense_mode) {
    if (!d->dense_grad || d->dense_rows < table_rows(d) - dense_lo_of(d)) return ANIREC_EINVAL;
    if (d->adam_row_lo < 0 || d->adam_row_hi < d->adam_row_lo || d->adam_row_hi > table_rows(d)) return ANIREC_EINVAL;
  }
  if (d->workspace_bytes < anirec_train_workspace_bytes_w(d->max_batch, d->arena_steps, dim))
    return ANIREC_EWORKSPACE;
  return ANIREC_OK;
}

// What a step of the lazy update launches besides fwd, head, bwd and the sparse step; ignored by the dense update.
struct StepFlags {
  bool catchup_first;  // the rows of this step's batch are not known to be current: a stand-alone catch-up launch
  bool fuse_next;      // the NEXT step's batch is in the prep arena: this step's launches also catch its rows up
  bool flush_after;    // a flush follows the step: its window is full, or the run ends with it
};

// The cadence of a run of steps walked in prepared blocks (a block: steps whose batches are all in the prep arena).
// Only a block's first step needs a catch-up launch of its own, every step but a block's last fuses the next batch's
// catch-up, and a flush follows every kLzWin steps and the last step of the run, so a run ends flushed.
struct Walk {
  int run_left = 0;              // steps of the run still to come
  int blk_len = 0, blk_pos = 0;  // the prepared block the next step belongs to
  int open = 0;                  // steps taken since the last flush
  void begin(int n_steps) {
    run_left = n_steps;
    blk_len = blk_pos = open = 0;
  }
  void block(int n_steps) {
    blk_len = n_steps;
    blk_pos = 0;
  }
  bool in_block() const { return run_left > 0 && blk_pos < blk_len; }
  StepFlags peek() const { return {blk_pos == 0, blk_pos + 1 < blk_len, open + 1 == kLzWin || run_left == 1}; }
  StepFlags next() {  // the flags of the next step, which is taken
    const StepFlags f = peek();
    open = f.flush_after ? 0 : open + 1;
    if (run_left > 0) --run_left;
    if (blk_pos < blk_len) ++blk_pos;
    return f;
  }
};

// The part of a handle (anirec_trainer, anirec_dist_stepper) the block scheduler works on.
struct RunHandle {
  anirec_train_desc d;
  TrainWs ws;
  hipGraphExec_t exec = nullptr;  // the captured block of graph_steps steps
  int graph_steps = 0;            // < 0: a capture failed, the handle runs eagerly from then on
  MetricArgs metrics = {};        // the Keras metrics of every step (mask 0: none)
};

// host: a metric set the kernels implement for this descriptor (AUC needs p in [0, 1]: the sigmoid head)
int check_metrics(const anirec_train_desc *d, uint32_t mask) {
  if (mask & ~kMetricBits) return ANIREC_EINVAL;
  if ((mask & ANIREC_METRIC_AUC) && d->activation != ANIREC_ACT_SIGMOID) return ANIREC_EINVAL;
  return ANIREC_OK;
}

// a handle's metric set; the captured graph holds the old kernel arguments: dropped
static int set_metrics(RunHandle *h, uint32_t mask, anirec_metric_acc *acc) {
  if (int e = check_metrics(&h->d, mask)) return e;
  h->metrics = (mask && acc) ? MetricArgs{mask, acc} : MetricArgs{};
  if (h->exec) (void)hipGraphExecDestroy(h->exec);
  h->exec = nullptr;
  if (h->graph_steps > 0) h->graph_steps = 0;
  return ANIREC_OK;
}

// Runs steps [first_step, first_step + n_steps) of h's descriptor, `step(stream, flags)` enqueuing the launches of one
// step.  With use_graph a block of G = min(32, arena_steps / 2) steps is captured once per handle and replayed: a
// replay starts with the prep of the G steps AFTER it (relative to the device cursor), so no host work falls between
// replays; the arena holds 2G steps.  The steps left over run eagerly, in arena-sized blocks prepared from the host —
// except after a replay, which has prepared them already.  A failed capture returns ANIREC_ECAPTURE with nothing of
// the run enqueued.
template <class Step>
static int run_blocks(RunHandle *h, hipStream_t s, int first_step, int n_steps, bool use_graph, Step step) {
  const anirec_train_desc *d = &h->d;
  int G = d->arena_steps / 2;
  if (G > 32) G = 32;
  // (stamped steps run eagerly)
  const bool graph = use_graph && s != nullptr && G >= 4 && n_steps >= G && !g_ticks_on && h->graph_steps >= 0;
  if (graph && !h->exec) {
    hipGraph_t g = nullptr;
    int e = ANIREC_ECAPTURE;
    if (hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed) == hipSuccess) {
      e = launch_prep(d, h->ws, G, G, true, s);  // steps cursor+G .. cursor+2G
      Walk walk;  // a run of G steps in one block of G: a replay leaves the tables up to date
      walk.begin(G);
      walk.block(G);
      for (int i = 0; i < G && !e; ++i) e = step(s, walk.next());
      if (hipStreamEndCapture(s, &g) != hipSuccess || !g) e = ANIREC_ECAPTURE;
    }
    if (!e && hipGraphInstantiate(&h->exec, g, nullptr, nullptr, 0) != hipSuccess) e = ANIREC_ECAPTURE;
    if (g) (void)hipGraphDestroy(g);
    if (e) {
      h->exec = nullptr;
      (void)hipGetLastError();
      return ANIREC_ECAPTURE;
    }
    h->graph_steps = G;
  }
  if (n_steps > 0 && (lazy_on(d) || lazy_users(d))) {
    const int e = lazy_begin(d, h->ws, first_step, s);
    if (e) return e;
  }
  int done = 0;
  if (graph) {
    const int e = launch_prep(d, h->ws, first_step, G, false, s);  // the first block; later ones by the graph
    if (e) return e;
    for (; n_steps - done >= G; done += G) ANIREC_HIP_CHECK(hipGraphLaunch(h->exec, s));
  }
  Walk walk;
  walk.begin(n_steps - done);
  while (done < n_steps) {
    int blk = n_steps - done;
    if (!graph) {  // (after replays the last one has prepared the tail)
      if (blk > d->arena_steps) blk = d->arena_steps;
      const int e = launch_prep(d, h->ws, first_step + done, blk, false, s);
      if (e) return e;
    }
    walk.block(blk);
    for (int i = 0; i < blk; ++i)
      if (const int e = step(s, walk.next())) return e;
    done += blk;
  }
  return ANIREC_OK;
}

// one step on one GPU: the dense update, or the lazy one with the launches its flags ask for
static int train_step(const anirec_train_desc *d, const TrainWs &w, hipStream_t s, StepFlags f, MetricArgs m) {
  const bool lazy = lazy_on(d);
  int e;
  if (lazy && f.catchup_first && (e = launch_lazy_catchup(d, w, s))) return e;
  if ((e = launch_fwd(d, w, s))) return e;
  if ((e = launch_head(d, w, s, lazy && f.fuse_next, m))) return e;
  if ((e = launch_bwd_only(d, w, s, lazy))) return e;
  if (!lazy) return launch_adam_full(d, w, s, 0);
  if ((e = launch_lazy_adam(d, w, s, f.fuse_next))) return e;
  return f.flush_after ? lazy_flush(d, w, s) : ANIREC_OK;
}

}  // namespace anirec

using namespace anirec;

extern "C" {

// c[pcap] | t[pcap] | {count,0,0,0}, pcap = max_batch rounded up to 4 floats (16-B aligned rows)
size_t anirec_packet_floats(int32_t max_batch) { return 2 * (size_t)packet_cap(max_batch) + 4; }

size_t anirec_train_lazy_bytes(int32_t rows) {
  if (rows < 1) return 0;
  return 2 * ((sizeof(int32_t) * (size_t)rows + 255) / 256 * 256) + sizeof(float) * (size_t)rows * ANIREC_LAZY_WINDOW;
}

size_t anirec_train_workspace_bytes_w(int32_t max_batch, int32_t arena_steps, int32_t dim) {
  if (max_batch < 1 || max_batch > ANIREC_MAX_BATCH || arena_steps < 2 || !dim_ok(dim)) return 0;
  return carve(nullptr, max_batch, arena_steps, dim).total;
}
size_t anirec_train_workspace_bytes(int32_t max_batch, int32_t arena_steps) {
  return anirec_train_workspace_bytes_w(max_batch, arena_steps, ANIREC_DIM);
}

int anirec_train_prep_w(const anirec_train_desc *d, int32_t dim, int32_t first_step, int32_t n_steps, void *stream) {
  int rc = check_desc(d, dim);
  if (rc) return rc;
  if (!d->user_idx || !d->anime_idx || !d->sched) return ANIREC_EINVAL;
  if (first_step < 0 || n_steps < 0 || first_step + n_steps > d->n_steps ||
      n_steps > d->arena_steps)
    return ANIREC_EINVAL;
  if (n_steps == 0) return ANIREC_OK;
  return launch_prep(d, carve(d->workspace, d->max_batch, d->arena_steps, dim), first_step, n_steps, false,
                     (hipStream_t)stream);
}
int anirec_train_prep(const anirec_train_desc *d, int32_t first_step, int32_t n_steps,
                      void *stream) {
  return anirec_train_prep_w(d, ANIREC_DIM, first_step, n_steps, stream);
}

int anirec_train_fwd_w(const anirec_train_desc *d, int32_t dim, void *stream) {
  int rc = check_desc(d, dim);
  if (rc) return rc;
  if (!d->user_idx || !d->anime_idx || !d->rating || !d->sched) return ANIREC_EINVAL;
  return launch_fwd(d, carve(d->workspace, d->max_batch, d->arena_steps, dim), (hipStream_t)stream);
}
int anirec_train_fwd(const anirec_train_desc *d, void *stream) { return anirec_train_fwd_w(d, ANIREC_DIM, stream); }

int anirec_train_head_w(const anirec_train_desc *d, int32_t dim, void *stream) {
  int rc = check_desc(d, dim);
  if (rc) return rc;
  if (!d->sched) return ANIREC_EINVAL;
  return launch_head(d, carve(d->workspace, d->max_batch, d->arena_steps, dim), (hipStream_t)stream);
}
int anirec_train_head(const anirec_train_desc *d, void *stream) { return anirec_train_head_w(d, ANIREC_DIM, stream); }

int anirec_train_bwd_w(const anirec_train_desc *d, int32_t dim, void *stream) {
  int rc = check_desc(d, dim);
  if (rc) return rc;
  return launch_bwd(d, carve(d->workspace, d->max_batch, d->arena_steps, dim), (hipStream_t)stream);
}
int anirec_train_bwd(const anirec_train_desc *d, void *stream) { return anirec_train_bwd_w(d, ANIREC_DIM, stream); }

int anirec_train_adam_w(const anirec_train_desc *d, int32_t dim, void *stream) {
  int rc = check_desc(d, dim);
  if (rc) return rc;
  return launch_adam_full(d, carve(d->workspace, d->max_batch, d->arena_steps, dim), (hipStream_t)stream, 0);
}
int anirec_train_adam(const anirec_train_desc *d, void *stream) { return anirec_train_adam_w(d, ANIREC_DIM, stream); }

int anirec_train_adam_part(const anirec_train_desc *d, int32_t which, void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  TrainWs w = carve(d->workspace, d->max_batch, d->arena_steps);
  hipStream_t s = (hipStream_t)stream;
  if ((which != 1 && which != 2) || d->dense_mode != 1) return ANIREC_EINVAL;
  // lazy user rows are only kept current by the run's cadence (anirec_dist_stepper_begin / _block): a part on its own
  // would update rows that are steps behind, or account into a window that was never opened
  if (lazy_users(d)) return ANIREC_EINVAL;
  return launch_adam_full(d, w, s, which);
}

// ---- multi-GPU step halves (one C call each; the caller issues the two collectives between them) ----------
// (the graph of anirec_dist_run holds a block of steps, collectives included)
struct anirec_dist_stepper : RunHandle {
  hipStream_t side = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  Walk walk;  // lazy user rows: where the step-by-step callers are in their run and prepared block
};

int anirec_dist_stepper_create(const anirec_train_desc *d, anirec_dist_stepper **out) {
  if (!out) return ANIREC_EINVAL;
  int rc = check_desc(d);
  if (rc) return rc;
  if (!d->dense_mode) return ANIREC_EINVAL;
  anirec_dist_stepper *h = new (std::nothrow) anirec_dist_stepper;
  if (!h) return ANIREC_EINVAL;
  h->d = *d;
  h->ws = carve(d->workspace, d->max_batch, d->arena_steps);
  if (hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&h->fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->join, hipEventDisableTiming) != hipSuccess) {
    anirec_dist_stepper_destroy(h);
    return ANIREC_ENODEVICE;
  }
  *out = h;
  return ANIREC_OK;
}

int anirec_dist_stepper_destroy(anirec_dist_stepper *h) {
  if (!h) return ANIREC_EINVAL;
  if (h->exec) (void)hipGraphExecDestroy(h->exec);
  if (h->fork) (void)hipEventDestroy(h->fork);
  if (h->join) (void)hipEventDestroy(h->join);
  if (h->side) (void)hipStreamDestroy(h->side);
  delete h;
  return ANIREC_OK;
}

// ---- the three parts of a multi-GPU step (the collectives go between them) ----------------------------------
// front: [lazy user rows: the catch-up of this batch's rows when no earlier step of the block has done it] + fwd
static int dist_front(anirec_dist_stepper *h, hipStream_t s, bool catchup_first) {
  int e;
  if (lazy_users(&h->d) && catchup_first && (e = launch_lazy_catchup(&h->d, h->ws, s))) return e;
  return launch_fwd(&h->d, h->ws, s);
}

// mid — after the all-gather of the head packets: head, bwd, and the densify pass that feeds the gradient
// collective.  User-sharded mode: the update of this rank's user rows needs nothing from the collective, so it is
// forked onto the stepper's side stream right behind bwd and runs beside densify + all-reduce: the dense Adam stream
// over the user rows, or — lazy user rows — the sparse step of the rows the batch touched (the catch-up of the next
// batch's rows rides in the head launch when `fuse_next`: its chunk table is in the arena).
static int dist_mid(anirec_dist_stepper *h, hipStream_t s, bool fuse_next) {
  const bool lz = lazy_users(&h->d);
  int e;
  if ((e = launch_head(&h->d, h->ws, s, lz && fuse_next, h->metrics))) return e;
  if ((e = launch_bwd_only(&h->d, h->ws, s, lz))) return e;
  if (h->d.dense_mode == 1) {
    ANIREC_HIP_CHECK(hipEventRecord(h->fork, s));
    ANIREC_HIP_CHECK(hipStreamWaitEvent(h->side, h->fork, 0));
    if ((e = lz ? launch_lazy_adam(&h->d, h->ws, h->side, fuse_next) : launch_adam_full(&h->d, h->ws, h->side, 1)))
      return e;
    ANIREC_HIP_CHECK(hipEventRecord(h->join, h->side));
  }
  return launch_densify(&h->d, h->ws, s);
}

// back — after the gradient collective: the rows that needed it + the step finish [+ lazy user rows: the flush of
// the window when `flush_after`]
static int dist_back(anirec_dist_stepper *h, hipStream_t s, bool flush_after) {
  int e;
  if (h->d.dense_mode == 1) {
    ANIREC_HIP_CHECK(hipStreamWaitEvent(s, h->join, 0));
    e = launch_adam_full(&h->d, h->ws, s, 2);
  } else {
    e = launch_adam_full(&h->d, h->ws, s, 0);
  }
  if (!e && flush_after && lazy_users(&h->d)) e = lazy_flush(&h->d, h->ws, s);
  return e;
}

// Callers that drive the step themselves (three C calls + their own collectives per step) say where they are:
// begin(first_step, n_steps) once per run — the tables are current there, a lazy window opens — and block(n) after
// every anirec_train_prep of n steps.  With lazy user rows both are REQUIRED (ANIREC_EINVAL from the step calls
// otherwise: a run that is never told where it ends would leave the tables behind); without, they are no-ops.
int anirec_dist_stepper_begin(anirec_dist_stepper *h, int32_t first_step, int32_t n_steps, void *stream) {
  if (!h || first_step < 0 || n_steps < 0 || first_step + n_steps > h->d.n_steps) return ANIREC_EINVAL;
  h->walk.begin(n_steps);
  if (lazy_users(&h->d) && n_steps > 0) return lazy_begin(&h->d, h->ws, first_step, (hipStream_t)stream);
  return ANIREC_OK;
}

int anirec_dist_stepper_block(anirec_dist_stepper *h, int32_t n_steps) {
  if (!h || n_steps < 0 || n_steps > h->d.arena_steps) return ANIREC_EINVAL;
  h->walk.block(n_steps);
  return ANIREC_OK;
}

// (the walk advances at the back of a step: front and mid look at the step it is at)
static bool outside_walk(const anirec_dist_stepper *h) { return lazy_users(&h->d) && !h->walk.in_block(); }

int anirec_dist_step_front(anirec_dist_stepper *h, void *stream) {
  if (!h || outside_walk(h)) return ANIREC_EINVAL;
  return dist_front(h, (hipStream_t)stream, h->walk.peek().catchup_first);
}

int anirec_dist_step_mid(anirec_dist_stepper *h, void *stream) {
  if (!h || outside_walk(h)) return ANIREC_EINVAL;
  return dist_mid(h, (hipStream_t)stream, h->walk.peek().fuse_next);
}

int anirec_dist_step_back(anirec_dist_stepper *h, void *stream) {
  if (!h || outside_walk(h)) return ANIREC_EINVAL;
  return dist_back(h, (hipStream_t)stream, h->walk.next().flush_after);
}

// ---- multi-GPU: the whole loop in the library, RCCL called from here -----------------------------------------
// The step sequence above driven from C: one call enqueues prep + n_steps x {fwd -> all-gather(packets) -> mid ->
// all-reduce | reduce-scatter(dense grad) -> back [-> all-gather(W rows)]} on the engine's stream, the collectives
// issued to RCCL on that same stream (no Python, no torch.distributed in the step).  RCCL is bound with dlopen — the
// copy the process has already loaded (torch's) when there is one — so the library has no link-time dependency on
// it and a box without RCCL still loads libanirec.
struct RcclApi {
  void *lib = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclReduceScatter) ReduceScatter = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
};
static RcclApi g_rccl;

static int rccl_bind(void *lib) {
  RcclApi a;
  a.lib = lib;
#define ANIREC_SYM(F)                                               \
  a.F = reinterpret_cast<decltype(a.F)>(dlsym(lib, "nccl" #F));     \
  if (!a.F) return ANIREC_ENODEVICE;
  ANIREC_SYM(GetUniqueId)
  ANIREC_SYM(CommInitRank)
  ANIREC_SYM(CommDestroy)
  ANIREC_SYM(AllGather)
  ANIREC_SYM(AllReduce)
  ANIREC_SYM(ReduceScatter)
  ANIREC_SYM(GroupStart)
  ANIREC_SYM(GroupEnd)
#undef ANIREC_SYM
  g_rccl = a;
  return ANIREC_OK;
}

int anirec_rccl_load(const char *path_host) {
  if (g_rccl.lib) return ANIREC_OK;
  if (path_host && path_host[0]) {
    void *l = dlopen(path_host, RTLD_NOW | RTLD_LOCAL);
    return l ? rccl_bind(l) : ANIREC_ENODEVICE;
  }
  static const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (int pass = 0; pass < 2; ++pass)  // first a copy that is already mapped (torch's), then a fresh load
    for (const char *nm : names) {
      void *l = dlopen(nm, RTLD_NOW | RTLD_LOCAL | (pass == 0 ? RTLD_NOLOAD : 0));
      if (l && rccl_bind(l) == ANIREC_OK) return ANIREC_OK;
    }
  return ANIREC_ENODEVICE;
}

int anirec_rccl_unique_id(char *id_host) {
  if (!id_host) return ANIREC_EINVAL;
  if (!g_rccl.lib) return ANIREC_ENODEVICE;
  ncclUniqueId id;
  if (g_rccl.GetUniqueId(&id) != ncclSuccess) return ANIREC_ECOMM;
  static_assert(sizeof(id) == ANIREC_RCCL_ID_BYTES, "ncclUniqueId size");
  memcpy(id_host, &id, sizeof(id));
  return ANIREC_OK;
}

struct anirec_dist_comm {
  ncclComm_t comm;
  int rank, world;
};

int anirec_dist_comm_create(const char *id_host, int32_t rank, int32_t world, anirec_dist_comm **out) {
  if (!id_host || !out || world < 1 || world > ANIREC_MAX_SEG || rank < 0 || rank >= world) return ANIREC_EINVAL;
  if (!g_rccl.lib) return ANIREC_ENODEVICE;
  anirec_dist_comm *c = new (std::nothrow) anirec_dist_comm;
  if (!c) return ANIREC_EINVAL;
  ncclUniqueId id;
  memcpy(&id, id_host, sizeof(id));
  c->rank = rank;
  c->world = world;
  if (g_rccl.CommInitRank(&c->comm, world, id, rank) != ncclSuccess) {  // collective: every rank calls it
    delete c;
    return ANIREC_ECOMM;
  }
  *out = c;
  return ANIREC_OK;
}

int anirec_dist_comm_destroy(anirec_dist_comm *c) {
  if (!c) return ANIREC_EINVAL;
  if (g_rccl.lib) (void)g_rccl.CommDestroy(c->comm);
  delete c;
  return ANIREC_OK;
}

#define ANIREC_RCCL_CHECK(expr)                      \
  do {                                               \
    if ((expr) != ncclSuccess) return ANIREC_ECOMM;  \
  } while (0)

// reduce-scatter form of the replicated tables: this rank's Adam only updates its row shard
static inline bool row_sharded(const anirec_train_desc *d) {
  return d->dense_mode == 2 && (d->adam_row_lo | d->adam_row_hi) != 0;
}

static int dist_one_step(anirec_dist_stepper *h, anirec_dist_comm *c, hipStream_t s, StepFlags f) {
  const anirec_train_desc *d = &h->d;
  int e;
  if ((e = dist_front(h, s, f.catchup_first))) return e;
  // BatchNorm sees the global batch: every rank's (c, t, count, mean, M2) packet, gathered in place
  const size_t pf = anirec_packet_floats(d->max_batch);
  ANIREC_RCCL_CHECK(g_rccl.AllGather(d->packets + pf * (size_t)c->rank, d->packets, pf, ncclFloat, c->comm, s));
  if ((e = dist_mid(h, s, f.fuse_next))) return e;
  float *g = d->dense_grad;
  const size_t nd = (size_t)d->dense_rows;
  if (row_sharded(d)) {
    // rows and self-coefficient sums of this rank's shard only, in place (dense_rows is a multiple of the world size)
    const size_t sr = nd / (size_t)c->world;
    ANIREC_RCCL_CHECK(g_rccl.GroupStart());
    ANIREC_RCCL_CHECK(g_rccl.ReduceScatter(g, g + (size_t)c->rank * sr * kDim, sr * kDim, ncclFloat, ncclSum, c->comm, s));
    ANIREC_RCCL_CHECK(g_rccl.ReduceScatter(g + nd * kDim, g + nd * kDim + (size_t)c->rank * sr, sr, ncclFloat, ncclSum,
                                           c->comm, s));
    ANIREC_RCCL_CHECK(g_rccl.GroupEnd());
  } else {
    ANIREC_RCCL_CHECK(g_rccl.AllReduce(g, g, nd * (kDim + 1), ncclFloat, ncclSum, c->comm, s));
  }
  if ((e = dist_back(h, s, f.flush_after))) return e;
  if (row_sharded(d)) {  // every rank updated its row shard: collect the updated rows of W (padded to whole shards)
    const size_t sr = nd / (size_t)c->world;
    ANIREC_RCCL_CHECK(g_rccl.AllGather(d->W + (size_t)c->rank * sr * kDim, d->W, sr * kDim, ncclFloat, c->comm, s));
  }
  return ANIREC_OK;
}

// use_graph: the blocks run_blocks captures hold their RCCL collectives and the side-stream fork / join too; every rank
// replays in lockstep.  If the capture or the instantiation fails the loop falls back to eager launches for good.
int anirec_dist_run(anirec_dist_stepper *h, anirec_dist_comm *c, int32_t first_step, int32_t n_steps, int32_t use_graph,
                    void *stream) {
  if (!h || !c || n_steps < 0 || first_step < 0 || first_step + n_steps > h->d.n_steps) return ANIREC_EINVAL;
  if (!g_rccl.lib) return ANIREC_ENODEVICE;
  if (c->world != h->d.n_seg || c->rank != h->d.my_seg) return ANIREC_EINVAL;
  if (!h->d.user_idx || !h->d.anime_idx || !h->d.rating || !h->d.sched || !h->d.dense_grad) return ANIREC_EINVAL;
  if (row_sharded(&h->d) && h->d.dense_rows % c->world) return ANIREC_EINVAL;
  const auto step = [h, c](hipStream_t s, StepFlags f) { return dist_one_step(h, c, s, f); };
  int e = run_blocks(h, (hipStream_t)stream, first_step, n_steps, use_graph != 0, step);
  if (e == ANIREC_ECAPTURE) {
    h->graph_steps = -1;
    e = run_blocks(h, (hipStream_t)stream, first_step, n_steps, false, step);
  }
  return e;
}

// ---- one GPU: the whole loop ------------------------------------------------------------------------------
struct anirec_trainer : RunHandle {};

int anirec_trainer_create(const anirec_train_desc *d, anirec_trainer **out) {
  return anirec_trainer_create_w(d, ANIREC_DIM, out);
}

// the handle carries the width (its carved workspace): _run, _set_metrics and _destroy are the same calls at every width
int anirec_trainer_create_w(const anirec_train_desc *d, int32_t dim, anirec_trainer **out) {
  if (!out) return ANIREC_EINVAL;
  int rc = check_desc(d, dim);
  if (rc) return rc;
  if (d->n_seg != 1 || d->dense_mode) return ANIREC_EINVAL;  // multi-GPU drives the step halves itself
  anirec_trainer *t = new (std::nothrow) anirec_trainer;
  if (!t) return ANIREC_EINVAL;
  t->d = *d;
  t->ws = carve(d->workspace, d->max_batch, d->arena_steps, dim);
  *out = t;
  return ANIREC_OK;
}

int anirec_trainer_destroy(anirec_trainer *t) {
  if (!t) return ANIREC_EINVAL;
  if (t->exec) (void)hipGraphExecDestroy(t->exec);
  delete t;
  return ANIREC_OK;
}

// Runs steps [first_step, first_step + n_steps); first_step must equal the device cursor (state->step_fwd).
int anirec_trainer_run(anirec_trainer *t, int32_t first_step, int32_t n_steps, int32_t use_graph,
                       void *stream) {
  if (!t || n_steps < 0 || first_step < 0 || first_step + n_steps > t->d.n_steps) return ANIREC_EINVAL;
  if (!t->d.user_idx || !t->d.anime_idx || !t->d.rating || !t->d.sched) return ANIREC_EINVAL;
  return run_blocks(t, (hipStream_t)stream, first_step, n_steps, use_graph != 0,
                    [t](hipStream_t s, StepFlags f) { return train_step(&t->d, t->ws, s, f, t->metrics); });
}

int anirec_trainer_set_metrics(anirec_trainer *t, uint32_t mask, anirec_metric_acc *acc) {
  if (!t) return ANIREC_EINVAL;
  return set_metrics(t, mask, acc);
}

int anirec_dist_stepper_set_metrics(anirec_dist_stepper *h, uint32_t mask, anirec_metric_acc *acc) {
  if (!h) return ANIREC_EINVAL;
  return set_metrics(h, mask, acc);
}

}  // extern "C"
