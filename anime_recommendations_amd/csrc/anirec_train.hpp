// What the units of the training path share (anirec_train*.hip; the map is in DESIGN.md, 4.1): the workspace layout,
// the kernel argument structs that more than one unit fills or reads, the measurement stamp, the small host predicates
// and the declarations of the host functions that are called across units.  A kernel is launched only from the unit that
// defines it: what crosses a file boundary is always a launch_* function, never a kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "anirec_dev.hpp"

namespace anirec {

// ------------------------------------------------------------------------------------
// workspace layout
// ------------------------------------------------------------------------------------
// Step constants written by workgroup 0 of the head kernel, read by bwd and adam.
struct StepPub {
  int slot, n_total, n_head_blocks, step;
  float alpha, mu, var, rs;
  float w, b, gamma, beta;
  float l2, pad0, pad1, pad2;
};


struct TrainWs {
  int cap, capC, arena_steps;
  int dim;                      // row width of the tables (floats): ANIREC_DIM unless carved by a *_w entry point
  float *su, *sa;               // [cap] row square sums from fwd
  float *dy;                    // [cap] d loss / d y from head
  // everything below this line is double-buffered by step parity (index p = step & 1)
  float *hpart;                 // [2][ANIREC_MAX_SEG * ceil(cap/256)][8] head partial sums
  size_t hpart_stride;          // floats per parity
  StepPub *pub;                 // [2] step constants published by head workgroup 0
  int32_t *sel;                 // step index of the last head launch (read by bwd / densify / adam)
  unsigned long long *ticks;    // [8][ANIREC_ADAM_BLOCKS][2] measurement stamps (fwd, head, bwd, adam, lazy catch-up,
                                // lazy adam, lazy flush, lazy reduce), behind the arena
  float *lzpart;                // [ANIREC_LAZY_WINDOW][2][ANIREC_ADAM_BLOCKS] lazy flush: per-step sum(W^2) block partials
  float *lzring;                // [ANIREC_LAZY_WINDOW][2] lazy: {n, bce mean} of the open window's steps (bce: the data
                                //   term of the descriptor's loss, whichever it is)
  float *regpart;               // [2][2][ANIREC_ADAM_BLOCKS]: user-row / anime-row sum(W^2) partials
  float *P;                     // [2][2*capC][dim] chunk partial rows
  float *S;                     // [2][2*capC]      chunk self-coefficient sums
  // arena slot s: nchunks[2] (4 ints), sidx[2][cap], oth[2][cap], chunks[2][capC] (int4)
  char *arena;
  size_t slot_bytes;
  size_t total;
};

__host__ __device__ inline int chunk_capacity(int cap) {
  int c = cap + cap / ANIREC_CHUNK + 2;
  return (c + 3) & ~3;
}

__host__ inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

__host__ __device__ inline int packet_cap(int max_batch) { return (max_batch + 3) & ~3; }

__host__ inline TrainWs carve(void *base, int cap, int arena_steps, int dim = kDim) {
  TrainWs w;
  w.dim = dim;
  w.cap = cap;
  w.capC = chunk_capacity(cap);
  w.arena_steps = arena_steps;
  size_t off = 0;
  char *b = (char *)base;
  auto take = [&](size_t bytes) {
    char *p = b + off;
    off += align_up(bytes);
    return p;
  };
  w.su = (float *)take(sizeof(float) * cap);
  w.sa = (float *)take(sizeof(float) * cap);
  w.dy = (float *)take(sizeof(float) * cap);
  w.hpart_stride = 8 * ANIREC_MAX_SEG * (size_t)((cap + 255) / 256);
  w.hpart = (float *)take(sizeof(float) * 2 * w.hpart_stride);
  w.pub = (StepPub *)take(sizeof(StepPub) * 2);
  w.sel = (int32_t *)take(sizeof(int32_t) * 4);
  w.regpart = (float *)take(sizeof(float) * 2 * 2 * ANIREC_ADAM_BLOCKS);
  w.P = (float *)take(sizeof(float) * 2 * 2 * (size_t)w.capC * dim);
  w.S = (float *)take(sizeof(float) * 2 * 2 * (size_t)w.capC);
  w.slot_bytes = align_up(16) + 2 * align_up(sizeof(int32_t) * 2 * (size_t)cap) +
                 align_up(sizeof(int4) * 2 * (size_t)w.capC);
  w.arena = take(w.slot_bytes * (size_t)arena_steps);
  w.ticks = (unsigned long long *)take(sizeof(unsigned long long) * 8 * 2 * ANIREC_ADAM_BLOCKS);
  w.lzpart = (float *)take(sizeof(float) * ANIREC_LAZY_WINDOW * 2 * ANIREC_ADAM_BLOCKS);
  w.lzring = (float *)take(sizeof(float) * ANIREC_LAZY_WINDOW * 2);
  w.total = off;
  return w;
}

struct Slot {
  int32_t *nchunks;  // [2] (+2 pad)
  int32_t *sidx;     // [2][cap]  batch-local rating index in row-sorted order
  int32_t *oth;      // [2][cap]  global W row of the other table, same order
  int4 *chunks;      // [2][capC] {global row, start, len, nch if first chunk of row else 0}
};

__host__ __device__ inline Slot slot_of(char *arena, size_t slot_bytes, int cap, int capC, int s) {
  char *p = arena + slot_bytes * (size_t)s;
  Slot r;
  size_t a0 = 256;
  size_t a1 = ((sizeof(int32_t) * 2 * (size_t)cap) + 255) / 256 * 256;
  r.nchunks = (int32_t *)p;
  r.sidx = (int32_t *)(p + a0);
  r.oth = (int32_t *)(p + a0 + a1);
  r.chunks = (int4 *)(p + a0 + 2 * a1);
  (void)capC;
  return r;
}

// ------------------------------------------------------------------------------------
// constants of more than one unit
// ------------------------------------------------------------------------------------
constexpr int kHeadThreads = 256;
constexpr int kHeadCols = 8;  // S1, S2, L, SE, sum dy*c, sum c, sum zh*c, sum zh
constexpr int kLzWin = ANIREC_LAZY_WINDOW;

// Measurement hook (bench.py): every workgroup leaves the 100 MHz constant-clock time of its first and last
// instruction; a kernel's duration is max(end) - min(start) over its workgroups — taken IN the step, on the batch the
// step really reads, with whatever the previous kernel left in the caches.
__device__ __forceinline__ void tick(unsigned long long *ticks, int which) {
  if (ticks == nullptr) return;  // kernel-uniform
  if (blockIdx.x >= ANIREC_ADAM_BLOCKS) return;  // a slot holds ANIREC_ADAM_BLOCKS stamp pairs (workgroup-uniform)
  if (which) {                   // the end stamp covers every wave of the workgroup and its stores
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if (threadIdx.x == 0) ticks[2 * (size_t)blockIdx.x + which] = __builtin_amdgcn_s_memrealtime();
}

// One row group (kD / 4 lanes: a half-wave at 128) per rating.  Returns dot products through references; all lanes
// of the group hold the totals.
template <int kD = kDim>
__device__ __forceinline__ void pair_dots(const float4 *W4, int urow, int arow, int l32, float &su,
                                          float &sa, float &dd) {
  constexpr int kG = kD / 4;
  const float4 u = W4[(size_t)urow * kG + l32];
  const float4 a = W4[(size_t)arow * kG + l32];
  float s0 = u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w;
  float s1 = a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
  float s2 = u.x * a.x + u.y * a.y + u.z * a.z + u.w * a.w;
  su = group_sum<kG>(s0);
  sa = group_sum<kG>(s1);
  dd = group_sum<kG>(s2);
}

__device__ __forceinline__ float cos_from_dots(float su, float sa, float dd) {
  const float ru = 1.0f / sqrtf(fmaxf(su, kL2nEps));
  const float ra = 1.0f / sqrtf(fmaxf(sa, kL2nEps));
  return dd * ru * ra;
}

// ------------------------------------------------------------------------------------
// kernel arguments that cross a unit: the head's, the metrics', the lazy update's
// ------------------------------------------------------------------------------------
struct HeadArgs {
  const anirec_state *state;
  const anirec_step *sched;
  const float *packets;  // n_seg packets
  size_t packet_floats;
  int n_seg, my_seg, cap, arena_steps;
  float *dy;             // [cap] d loss / d y of this rank's ratings
  float *hpart;          // [2][n_seg*blocks_per_seg][8]
  size_t hpart_stride;
  StepPub *pub;          // [2]
  int32_t *sel;
  float l2;
  unsigned long long *ticks;
};

// ---- Keras metrics (include/anirec.h, ANIREC_METRIC_*): the metrics instantiations of the head and of validation
// add the requested kinds to a caller-owned anirec_metric_acc; the default instantiations never see these
struct MetricArgs {
  uint32_t mask;  // ANIREC_METRIC_* bits, non-zero (wave-uniform: a kernel argument)
  anirec_metric_acc *acc;
};
constexpr int kMetricKinds = ANIREC_METRIC_KINDS;
constexpr int kAucBins = ANIREC_AUC_BINS;
constexpr uint32_t kMetricBits = (1u << (kMetricKinds + 1)) - 1;  // every ANIREC_METRIC_* bit

struct LazyState {
  int32_t *row_step;  // [rows] the step every row has been updated to (rows are current at the window's start)
  int32_t *mark;      // [rows] t + 1 for the rows batch t touched (written by fwd(t))
  float *rowsq;       // [rows][kLzWin] sum(W_s^2) of the row for the window's steps it has already taken
};
__host__ __device__ inline LazyState lazy_carve(void *base, int rows) {
  const size_t col = (sizeof(int32_t) * (size_t)rows + 255) / 256 * 256;
  LazyState z;
  z.row_step = (int32_t *)base;
  z.mark = (int32_t *)((char *)base + col);
  z.rowsq = (float *)((char *)base + 2 * col);
  return z;
}

struct LazyArgs {
  float *W, *M, *V;
  int rows, n_user_rows;
  LazyState z;
  const anirec_step *sched;
  int n_steps;
  anirec_state *state;
  int32_t *w0;  // device word: first step of the open window
  float two_l2, l2;
  char *arena;
  size_t slot_bytes;
  int cap, capC, arena_steps;
  float *lzpart, *lzring, *regpart;
  int tables;   // 2: both tables are updated lazily (one GPU); 1: the user rows only (user-sharded multi-GPU step: the
                // replicated anime rows take their dense update behind the all-reduce every step)
  int lazy_rows;  // rows [0, lazy_rows) are the lazily updated ones (all rows, or the user rows)
  int split;      // k_lazy_flush: workgroups [0, split) take the user rows, [split, grid) the anime rows
  int cu_lo;      // catch-up workgroups riding in another kernel's launch: they cover chunk-grid blocks [cu_lo, ...)
  int n_sparse;   // k_lazy_adam: workgroups [0, n_sparse) take the sparse step, the others a catch-up slice
  unsigned long long *ticks;
};

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
static inline int table_rows(const anirec_train_desc *d) { return d->n_user_rows + d->n_anime_rows; }
// first table row whose gradient travels through the dense buffer
static inline int dense_lo_of(const anirec_train_desc *d) { return d->dense_mode == 2 ? 0 : d->n_user_rows; }

// ---- which update the descriptor asks for ----
static inline bool lazy_on(const anirec_train_desc *d) {
  return d->lazy != 0 && d->lazy_state != nullptr && d->dense_mode == 0 && d->n_seg == 1;
}
// the user-sharded multi-GPU step with lazily updated user rows (the replicated anime rows stay dense: their
// gradient is summed over the ranks every step and most of them are touched by the global batch anyway)
static inline bool lazy_users(const anirec_train_desc *d) {
  return d->lazy != 0 && d->lazy_state != nullptr && d->dense_mode == 1;
}

// grid of the lazy kernels that walk the chunk table (a half-wave per chunk slot of the lazily updated tables)
static inline int lazy_chunk_grid(const anirec_train_desc *d, const TrainWs &w) {
  return ((lazy_users(d) ? 1 : 2) * w.capC + 7) / 8;
}

// The catch-up of the next batch's rows is cut in two slices of the chunk grid: blocks [0, head_share) ride in the
// head launch, the rest beside the sparse step in k_lazy_adam's.  The user chunks come first in that grid and are
// where the work is (the anime rows a batch touches are mostly current already).  Measured (S109M, one box,
// fwd + head + bwd + lazy_adam by the in-kernel stamps): share 0 % (round 3's place: everything behind bwd) 37.9 us,
// 35 % 34.8, 50 % 35.9, 65 % 36.2, 100 % 36.7 — the head launch, at the head's 109 VGPRs, holds four waves per
// SIMD and its own forty workgroups leave it after 7 us; more than ~3 500 rows in it only move the tail from one
// launch to the other.
constexpr int kCatchupHeadPct = 35;
static inline int catchup_head_share(const anirec_train_desc *d, const TrainWs &w) {
  return (int)((long long)lazy_chunk_grid(d, w) * kCatchupHeadPct / 100);
}

// measurement hook armed (anirec_train_stage_ticks): kernels stamp their workgroups' start / end times
extern bool g_ticks_on;  // (anirec_train.hip)
static inline unsigned long long *ticks_of(const TrainWs &w, int kernel) {
  return g_ticks_on ? w.ticks + (size_t)kernel * 2 * ANIREC_ADAM_BLOCKS : nullptr;
}

// ---- what is called across units; each has its one definition in the unit named --------------------------------
// anirec_train.hip: the step's kernels outside the head
int ticks_collect(const TrainWs &w, int kernel, hipStream_t s);
LazyArgs lazy_args(const anirec_train_desc *d, const TrainWs &w, int ticks_slot);
int launch_prep(const anirec_train_desc *d, const TrainWs &w, int first_step, int n_steps, bool relative_to_cursor,
                hipStream_t s);
int launch_fwd(const anirec_train_desc *d, const TrainWs &w, hipStream_t s);
int launch_bwd_only(const anirec_train_desc *d, const TrainWs &w, hipStream_t s, bool lazy = false);
int launch_bwd(const anirec_train_desc *d, const TrainWs &w, hipStream_t s);
int launch_densify(const anirec_train_desc *d, const TrainWs &w, hipStream_t s);
int launch_adam_full(const anirec_train_desc *d, const TrainWs &w, hipStream_t s, int which);
int lazy_begin(const anirec_train_desc *d, const TrainWs &w, int first_step, hipStream_t s);
int launch_lazy_catchup(const anirec_train_desc *d, const TrainWs &w, hipStream_t s);
int launch_lazy_adam(const anirec_train_desc *d, const TrainWs &w, hipStream_t s, bool fuse_next);
int lazy_flush(const anirec_train_desc *d, const TrainWs &w, hipStream_t s);
// anirec_train_head.hip, and the m.mask != 0 case it hands to anirec_train_head_metrics.hip
int launch_head(const anirec_train_desc *d, const TrainWs &w, hipStream_t s, bool fuse_next = false, MetricArgs m = {});
void launch_head_metrics(const anirec_train_desc *d, const HeadArgs &a, const LazyArgs &z, int n_head, int extra,
                         MetricArgs m, hipStream_t s);
// anirec_train_run.hip: what a descriptor and a metric set must satisfy
int check_opt(const anirec_train_desc *d);
int check_desc(const anirec_train_desc *d, int dim = kDim);
int check_metrics(const anirec_train_desc *d, uint32_t mask);

}  // namespace anirec
