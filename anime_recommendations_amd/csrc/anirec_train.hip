// Training hot path of libanirec for gfx950 (MI355X).
//
// Replaces the Keras train step driven by model.fit (reference
// neural_network/neural_network.py:210-217, graph at :66-106):
//
//   prep  one workgroup per (step, table): LDS radix sort of the batch by table row,
//         runs cut into chunks of <= ANIREC_CHUNK ratings  (TF: IndexedSlices ->
//         unsorted_segment_sum densification of the gather gradients)
//   fwd   half-wave per rating: coalesced 512-B gathers of U[ui], A[ai], three dot-128
//         reductions by wavefront shuffles -> c, sum(u^2), sum(a^2)
//   head  one workgroup per 256 ratings: batch mean/variance recomputed per workgroup,
//         Dense(1) -> BatchNorm(batch stats) -> activation -> loss (anirec_train_desc::activation / ::loss; one
//         instantiation per pair, the default sigmoid + BCE as it always was), d loss/d y, partial sums; with a
//         handle's metric set (anirec_trainer_set_metrics) k_head_metrics also accumulates the Keras metrics
//   bwd   half-wave per chunk: weighted sum of the OTHER table's rows, accumulated in
//         registers in a fixed order, one coalesced 512-B store per chunk (no float atomics).  The anime table's
//         chunk slots are the first of the grid (bwd and the lazy sparse step): the popular anime rows own the full
//         chunks and the many-chunk rows, the longest chains of both launches, and start with the launch.  Every
//         reader of a chunk table asks for the count word and the chunk record in one round trip (record index
//         clamped into the table's slots; a record past the count is dropped unread).
//   adam  half-wave per table row, dense: g = chunk sums - s*W + 2*l2*W, Keras-2.12 Adam,
//         emits sum(W_new^2) partials for the L2 loss term.  HBM-bound: 24 B/element
//         (+512 B per touched row) instead of 28 because the dense gradient never exists.
//         Workgroup 0 finishes the step (Adam on the 4 head scalars, moving stats, History metrics, step cursor).
//         Per-step scratch (chunk partials, row map, head partials, step constants, L2 partials) is
//         double-buffered by step parity: the multi-GPU step forks the user-row Adam onto a side stream beside the
//         densify pass + collective, and nothing of step t+1 can then overwrite what step t still reads.
//
// All kernels read the step index from device memory so one captured hipGraph replays for every step:
// fwd/head(t) from anirec_state::step_fwd (bumped by the finish of step t-1), bwd/densify/adam(t) from the word
// head(t) publishes (TrainWs::sel).  Each word has exactly one writer that runs strictly before its readers.
//
// Tried on the GPU and dropped (round 2): cutting the dense update in two launches — hot(t): the rows batch t+1
// touches, rest(t): everything else — so that fwd/head/bwd(t+1) could run beside the long rest(t) stream.  Bit-
// identical results, but no faster: as a second hipGraph branch or on a second stream every cross-branch edge
// costs ~12 us on this stack (rocprofv3 trace: 12-14 us gaps at each fork / join), more than the 29 us of small
// kernels it hides once the extra hot launch (13 us) is paid; fused INTO the rest launch (256-1024 workgroups
// running fwd -> barrier -> head -> barrier -> bwd beside the stream) the latency-bound chain crawls behind the
// bandwidth-saturating stream (270-400 us per step against 232).
//
// This unit holds the step's kernels outside the head — prep, fwd, bwd, the dense update, the lazy window — with their
// argument builders and launchers.  The head, validation, the self-tests and the host loop are units of their own
// (anirec_train_head.hip, _head_metrics, _eval, _util, _run; the map is in DESIGN.md, 4.1).
#include <hip/hip_runtime.h>

#include "anirec_train.hpp"
#include "anirec_train_lazy.hpp"

namespace anirec {

// ------------------------------------------------------------------------------------
// prep: stable LSD radix sort (8-bit digits) of one batch in LDS + chunk table
// ------------------------------------------------------------------------------------
constexpr int kSortThreads = 1024;
constexpr int kSortWaves = kSortThreads / 64;
constexpr int kSortMax = ANIREC_MAX_BATCH;       // 16384
constexpr int kPerThread = kSortMax / kSortThreads;  // 16

// exclusive prefix sum over the block; returns this thread's offset, total via *total
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *wsum /*[16]*/,
                                                    uint32_t *total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kSortWaves; ++k) {
    uint32_t s = wsum[k];
    if (k < w) base += s;
    tot += s;
  }
  if (total) *total = tot;
  return base + inc - v;
}

struct PrepArgs {
  const int32_t *user_idx, *anime_idx;
  const anirec_step *sched;
  int first_step;               // absolute first step, or relative to *cursor when cursor != nullptr
  const anirec_state *cursor;   // device cursor (graph replay): step = cursor->step_fwd + first_step + ...
  int n_steps_total;            // steps beyond the schedule are skipped
  int n_user_rows, n_anime_rows;
  int cap, capC, arena_steps;
  char *arena;
  size_t slot_bytes;
};

__global__ __launch_bounds__(kSortThreads) void k_prep(PrepArgs a) {
  __shared__ uint32_t keys[kSortMax];             // 64 KB
  __shared__ uint16_t vals[kSortMax];             // 32 KB (later: segment heads)
  __shared__ __attribute__((aligned(16))) uint32_t hist[256 * kSortWaves];  // 16 KB
  __shared__ uint32_t wsum[kSortWaves];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int step = (a.cursor ? a.cursor->step_fwd : 0) + a.first_step + (blockIdx.x >> 1);
  if (step >= a.n_steps_total) return;  // block-uniform
  const int T = blockIdx.x & 1;  // 0: sort by user row, 1: by anime row
  const anirec_step sc = a.sched[step];
  const int nb = min(sc.count, a.cap);
  const int base = sc.start;
  const int32_t *ksrc = T == 0 ? a.user_idx : a.anime_idx;
  const int32_t *osrc = T == 0 ? a.anime_idx : a.user_idx;
  const int nrows = T == 0 ? a.n_user_rows : a.n_anime_rows;
  const int row_off = T == 0 ? 0 : a.n_user_rows;     // global W row of key
  const int oth_off = T == 0 ? a.n_user_rows : 0;     // global W row of other index
  Slot sl = slot_of(a.arena, a.slot_bytes, a.cap, a.capC, step % a.arena_steps);

  // elements are dealt to waves in contiguous blocks so (wave, iteration, lane) order
  // == position order (needed for stability)
  const int npad = (nb + kSortThreads - 1) / kSortThreads * kSortThreads;
  const int per_wave = npad / kSortWaves;  // multiple of 64
  const int iters = per_wave / 64;         // <= 16

  for (int e = tid; e < npad; e += kSortThreads) {
    keys[e] = e < nb ? (uint32_t)ksrc[base + e] : 0xFFFFFFFFu;
    vals[e] = (uint16_t)e;
  }
  __syncthreads();

  int bits = 1;
  while (bits < 32 && (1u << bits) < (uint32_t)nrows) ++bits;
  const int npass = (bits + 7) / 8;

  volatile uint32_t *vh = hist;
  for (int pass = 0; pass < npass; ++pass) {
    const int shift = pass * 8;
    for (int i = tid; i < 256 * kSortWaves; i += kSortThreads) hist[i] = 0;
    __syncthreads();
    uint32_t k[kPerThread];
    uint16_t v[kPerThread];
    uint16_t off[kPerThread];
#pragma unroll
    for (int it = 0; it < kPerThread; ++it) {
      if (it < iters) {
        const int e = w * per_wave + it * 64 + lane;
        k[it] = keys[e];
        v[it] = vals[e];
        const uint32_t d = (k[it] >> shift) & 255u;
        // lanes of this wave holding the same digit
        unsigned long long peers = ~0ull;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          const bool bit = (d >> b) & 1u;
          const unsigned long long bal = __ballot(bit);
          peers &= bit ? bal : ~bal;
        }
        const unsigned long long lt = (1ull << lane) - 1ull;
        const uint32_t rank = __popcll(peers & lt);
        const uint32_t cnt = __popcll(peers);
        const uint32_t old = vh[d * kSortWaves + w];  // all peers read the same word
        if (rank == 0) vh[d * kSortWaves + w] = old + cnt;
        off[it] = (uint16_t)(old + rank);
      }
    }
    __syncthreads();
    // exclusive scan of hist in (digit-major, wave-minor) order: 4 entries per thread
    {
      uint4 h = *reinterpret_cast<uint4 *>(&hist[tid * 4]);
      uint32_t s = h.x + h.y + h.z + h.w;
      uint32_t b0 = block_excl_scan(s, wsum, nullptr);
      uint4 o;
      o.x = b0;
      o.y = b0 + h.x;
      o.z = o.y + h.y;
      o.w = o.z + h.z;
      *reinterpret_cast<uint4 *>(&hist[tid * 4]) = o;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kPerThread; ++it) {
      if (it < iters) {
        const uint32_t d = (k[it] >> shift) & 255u;
        const uint32_t dst = hist[d * kSortWaves + w] + off[it];
        keys[dst] = k[it];
        vals[dst] = v[it];
      }
    }
    __syncthreads();
  }

  // sorted order out: rating index and the other table's global row
  for (int p = tid; p < nb; p += kSortThreads) {
    const int v = vals[p];
    sl.sidx[T * a.cap + p] = v;
    sl.oth[T * a.cap + p] = osrc[base + v] + oth_off;
  }
  __syncthreads();

  // segment heads (first position of each distinct row), compacted into heads[]
  uint16_t *heads = vals;
  uint32_t nseg = 0;
  {
    const int p0 = tid * kPerThread;
    uint32_t flags = 0, cnt = 0;
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
      const int p = p0 + q;
      if (p < nb) {
        const bool h = (p == 0) || (keys[p] != keys[p - 1]);
        if (h) {
          flags |= 1u << q;
          ++cnt;
        }
      }
    }
    uint32_t o = block_excl_scan(cnt, wsum, &nseg);
    __syncthreads();  // everyone has read vals/keys neighbours before heads overwrite vals
#pragma unroll
    for (int q = 0; q < kPerThread; ++q)
      if (flags & (1u << q)) heads[o++] = (uint16_t)(p0 + q);
  }
  __syncthreads();

  // chunks per segment -> exclusive scan -> emit
  {
    const int h0 = tid * kPerThread;
    uint32_t nch[kPerThread];
    uint32_t cnt = 0;
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
      const uint32_t h = h0 + q;
      nch[q] = 0;
      if (h < nseg) {
        const int s0 = heads[h];
        const int s1 = (h + 1 < nseg) ? heads[h + 1] : nb;
        nch[q] = (uint32_t)((s1 - s0 + ANIREC_CHUNK - 1) / ANIREC_CHUNK);
        cnt += nch[q];
      }
    }
    uint32_t total = 0;
    uint32_t cb = block_excl_scan(cnt, wsum, &total);
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
      const uint32_t h = h0 + q;
      if (h < nseg) {
        const int s0 = heads[h];
        const int s1 = (h + 1 < nseg) ? heads[h + 1] : nb;
        const int row = (int)keys[s0] + row_off;
        for (uint32_t j = 0; j < nch[q]; ++j) {
          const int st = s0 + (int)j * ANIREC_CHUNK;
          int4 rec;
          rec.x = row;
          rec.y = st;
          rec.z = min(ANIREC_CHUNK, s1 - st);
          rec.w = j == 0 ? (int)nch[q] : 0;
          sl.chunks[T * a.capC + cb + j] = rec;
        }
        cb += nch[q];
      }
    }
    if (tid == 0) sl.nchunks[T] = (int)total;
  }
}

// ------------------------------------------------------------------------------------
// fwd: embedding lookup + L2-normalised dot
// ------------------------------------------------------------------------------------
struct FwdArgs {
  const float *W;
  int n_user_rows;
  const int32_t *user_idx, *anime_idx;
  const float *rating;
  const anirec_step *sched;
  const anirec_state *state;
  float *pk_c, *pk_t;
  int32_t *pk_count;
  float *su, *sa;
  int cap;
  int32_t *touched;  // lazy dense Adam: [rows], step + 1 for every row the batch touches (or nullptr)
  unsigned long long *ticks;  // measurement hook: [gridDim.x][2] start / end stamps per workgroup, or nullptr
};

// the forward pass of one workgroup: a row group (a half-wave at 128) per rating
template <int kD = kDim>
__device__ __forceinline__ void fwd_block(const FwdArgs &a, const anirec_step sc, int vblk, int step) {
  constexpr int kG = kD / 4;
  const int nb = min(sc.count, a.cap);
  const int per_blk = blockDim.x / kG;
  const int i = vblk * per_blk + (threadIdx.x / kG);
  if (vblk == 0 && threadIdx.x == 0) a.pk_count[0] = nb;
  if (i >= nb) return;
  const int l32 = threadIdx.x & (kG - 1);
  const int g = sc.start + i;
  const int ur = a.user_idx[g];
  const int ar = a.anime_idx[g] + a.n_user_rows;
  float su, sa, dd;
  pair_dots<kD>(reinterpret_cast<const float4 *>(a.W), ur, ar, l32, su, sa, dd);
  if (l32 == 0) {
    const float c = cos_from_dots(su, sa, dd);
    const float t = a.rating[g];
    a.pk_c[i] = c;
    a.pk_t[i] = t;
    a.su[i] = su;
    a.sa[i] = sa;
    // lazy dense Adam: the batch's rows are marked HERE, two kernels before the catch-up of the next batch's rows
    // (which rides in this step's head launch) asks which of them the sparse step of this batch will bring up to date
    if (a.touched != nullptr) {
      a.touched[ur] = step + 1;
      a.touched[ar] = step + 1;
    }
  }
}

// 1024 / kD ratings per workgroup.  The stamps are taken at 128 only (anirec_train_stage_ticks refuses the other widths).
template <int kD = kDim>
__global__ __launch_bounds__(256) void k_fwd(FwdArgs a) {
  if constexpr (kD == kDim) tick(a.ticks, 0);
  const int step = a.state->step_fwd;
  fwd_block<kD>(a, a.sched[step], blockIdx.x, step);
  if constexpr (kD == kDim) tick(a.ticks, 1);
}

// Multi-GPU only: (mean, M2) of this rank's z = w*c + b values, two-pass, written next to the
// count in the packet tail so that the all-gathered packets carry every rank's statistics.
__global__ __launch_bounds__(1024) void k_seg_stats(float *pk, int pcap, int cap,
                                                    const anirec_state *st) {
  __shared__ float scratch[16];
  const int cnt = min(reinterpret_cast<const int32_t *>(pk + 2 * (size_t)pcap)[0], cap);
  const float w = st->w, b = st->b;
  float r[1] = {0.f};
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) r[0] += pk[i] * w + b;
  block_sum<1>(r, scratch);
  const float mean = cnt > 0 ? r[0] / (float)cnt : 0.f;
  r[0] = 0.f;
  for (int i = threadIdx.x; i < cnt; i += blockDim.x) {
    const float d = (pk[i] * w + b) - mean;
    r[0] += d * d;
  }
  block_sum<1>(r, scratch);
  if (threadIdx.x == 0) {
    pk[2 * (size_t)pcap + 1] = mean;
    pk[2 * (size_t)pcap + 2] = r[0];
  }
}

// ------------------------------------------------------------------------------------
// bwd: per-chunk weighted row sums
// ------------------------------------------------------------------------------------
struct BwdArgs {
  const float *W;
  const StepPub *pub;    // [2]
  const int32_t *sel;
  const float *hpart;
  size_t hpart_stride;
  int rows;              // table rows: stride of the two row maps
  char *arena;
  size_t slot_bytes;
  int cap, capC;
  const float *pk_c;     // this rank's c
  const float *dy, *su, *sa;
  float *P, *S;
  int32_t *rowmap;
  int rowmap_lo;     // rows below it get no row-map word (user-sharded lazy mode: nobody would read or clear it)
  int arena_steps;
  unsigned long long *ticks;
};

// How a chunk (<= ANIREC_CHUNK contributions) sits on the kD / 4 lanes of its row group: lane l holds contributions
// l, l + kG, ... — one per lane at 128 (a half-wave) and at 256 (a wave, the upper half idle), four / two at 32 / 64.
template <int kD>
struct BwdGeom {
  static constexpr int kG = kD / 4;                                              // lanes of a row group
  static constexpr int kC = kG >= ANIREC_CHUNK ? 1 : ANIREC_CHUNK / kG;          // contributions a lane holds
  static constexpr int kRpb = 256 / kG;                                          // row groups per workgroup
};

// element `slot` (group-uniform) of a lane's per-contribution values; one element: the value itself
template <int kC, typename T>
__device__ __forceinline__ T pick(const T (&v)[kC], int slot) {
  T r = v[0];
#pragma unroll
  for (int k = 1; k < kC; ++k) r = slot == k ? v[k] : r;
  return r;
}

// what one row group needs for its chunk, requested as early as possible
template <int kC>
struct BwdPre {
  bool active;
  int T, c, len, i[kC], o[kC];
  int4 rec;
  float ci[kC], dyi[kC], su[kC], sa[kC];
  float4 r0[4];
};

template <int kD = kDim>
__device__ __forceinline__ void bwd_prefetch(const BwdArgs &a, int slot, int vblk, BwdPre<BwdGeom<kD>::kC> &x) {
  constexpr int kG = BwdGeom<kD>::kG, kC = BwdGeom<kD>::kC;
  const int l = threadIdx.x & (kG - 1);
  const int hw = vblk * BwdGeom<kD>::kRpb + (threadIdx.x / kG);
  // The anime table's chunk slots come first in the grid: its popular rows own the full 32-contribution chunks, the
  // longest chains of the launch, and those must not start in the dispatcher's second pass over the CUs.  Only the
  // workgroup -> (table, chunk) map is this; the chunk index gc = T capC + c that P / S / the row map use is not.
  x.T = hw < a.capC ? 1 : 0;
  x.c = hw - (1 - x.T) * a.capC;
  Slot sl = slot_of(a.arena, a.slot_bytes, a.cap, a.capC, slot);
  const float4 *W4 = reinterpret_cast<const float4 *>(a.W);
  // the count word and the chunk record in ONE round trip (both addresses hang on the step index alone): the record
  // index is clamped into the table's slots, and a record past the count is dropped unread
  int4 rec = sl.chunks[x.T * a.capC + min(x.c, a.capC - 1)];
  int nT = sl.nchunks[x.T];
  // (both loads are issued here: hipcc would sink the record's behind the test of the count)
  asm volatile("" : "+v"(nT), "+v"(rec.x), "+v"(rec.y), "+v"(rec.z), "+v"(rec.w));
  x.active = hw < 2 * a.capC && x.c < nT;
  x.len = 0;
  x.rec = make_int4(0, 0, 0, 0);
#pragma unroll
  for (int k = 0; k < kC; ++k) {
    x.i[k] = x.o[k] = 0;
    x.ci[k] = x.dyi[k] = 0.f;
    x.su[k] = x.sa[k] = 1.f;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) x.r0[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (x.active) {
    x.rec = rec;
    x.len = x.rec.z;
    // lane j < len holds contribution j of the chunk (+ j + kG, ... at the narrow widths); the rest replicate the
    // last one with weight 0 so every shuffle source is a valid row
#pragma unroll
    for (int k = 0; k < kC; ++k) {
      const int pos = x.rec.y + min(l + k * kG, x.len - 1);
      x.i[k] = sl.sidx[x.T * a.cap + pos];
      x.o[k] = sl.oth[x.T * a.cap + pos];
      x.ci[k] = a.pk_c[x.i[k]];
      x.dyi[k] = a.dy[x.i[k]];
      x.su[k] = a.su[x.i[k]];
      x.sa[k] = a.sa[x.i[k]];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) x.r0[q] = W4[(size_t)__shfl(x.o[0], q, kG) * kG + l];
  }
}

// mean(d zhat), mean(d zhat * zhat) numerators from the head partials: every row group sums them itself, lane l the
// partials l, l + kG, ... in that order, then the fixed butterfly — no LDS, no barrier (round 2 reduced them per
// workgroup through LDS: two barriers that every gather of the kernel had to wait behind)
struct BwdMeans {
  float2 v[2];
};
template <int kG = kRowVec>
__device__ __forceinline__ void bwd_means_issue(const float *hpart, int n_head_blocks, BwdMeans &x) {
  const int l = threadIdx.x & (kG - 1);
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int k = l + kG * q;
    x.v[q] = k < n_head_blocks ? *reinterpret_cast<const float2 *>(hpart + (size_t)k * kHeadCols) : make_float2(0.f, 0.f);
  }
}
template <int kG = kRowVec>
__device__ __forceinline__ void bwd_means_finish(const float *hpart, int n_head_blocks, const BwdMeans &x, float (&m)[2]) {
  const int l = threadIdx.x & (kG - 1);
  m[0] = x.v[0].x + x.v[1].x;
  m[1] = x.v[0].y + x.v[1].y;
  // at 128: more than 64 head workgroups, multi-GPU global batches only
  for (int k = l + 2 * kG; k < n_head_blocks; k += kG) {
    m[0] += hpart[(size_t)k * kHeadCols + 0];
    m[1] += hpart[(size_t)k * kHeadCols + 1];
  }
  m[0] = group_sum<kG>(m[0]);
  m[1] = group_sum<kG>(m[1]);
}

template <int kD = kDim, int kRows = 8>  // kRows: gathered rows in flight per row group
__device__ __forceinline__ void bwd_chunk(const BwdArgs &a, const StepPub &pub, int par, const float (&m)[2],
                                          const BwdPre<BwdGeom<kD>::kC> &x) {
  if (!x.active) return;
  constexpr int kG = BwdGeom<kD>::kG, kC = BwdGeom<kD>::kC;
  const int l = threadIdx.x & (kG - 1);
  const int T = x.T, c = x.c, len = x.len;
  const int4 rec = x.rec;
  const float4 *W4 = reinterpret_cast<const float4 *>(a.W);
  const float Bf = (float)pub.n_total;
  const float m1 = pub.gamma * m[0] / Bf;
  const float m2 = pub.gamma * m[1] / Bf;
  // A batch of one: z is its own mean and d loss / d z is exactly 0 (so the reference, so the oracle).  The expression
  // below gives the difference of two roundings of dy * gamma there (the product contracted into the subtraction, and
  // the product rounded in m1), 1e-7 after rs: a gradient Adam's epsilon lets move an element whose own L2 gradient is
  // as small by 2e-6 (tests/test_train_edges_gpu.py, tiny_ragged at width 32).
  const bool one = pub.n_total == 1;

  float cf[kC], sf[kC];
#pragma unroll
  for (int k = 0; k < kC; ++k) {
    const float ci = x.ci[k], dyi = x.dyi[k], su = x.su[k], sa = x.sa[k];
    // closed-form backward of BatchNorm + Dense(1) + normalised dot for rating i
    const float z = ci * pub.w + pub.b;
    const float zh = (z - pub.mu) * pub.rs;
    const float dz = one ? 0.f : (dyi * pub.gamma - m1 - zh * m2) * pub.rs;
    const float dc = dz * pub.w;
    const float ru = 1.0f / sqrtf(fmaxf(su, kL2nEps));
    const float ra = 1.0f / sqrtf(fmaxf(sa, kL2nEps));
    cf[k] = dc * ru * ra;
    const float sown = T == 0 ? su : sa;
    const float rown = T == 0 ? ru : ra;
    sf[k] = sown >= kL2nEps ? dc * ci * rown * rown : 0.f;
    if (l + k * kG >= len) {
      cf[k] = 0.f;
      sf[k] = 0.f;
    }
  }
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int q = 0; q < 4; ++q) {  // contributions 0..3 (rows already here; weight 0 past len)
    const float cq = __shfl(cf[0], q, kG);
    acc.x += cq * x.r0[q].x;
    acc.y += cq * x.r0[q].y;
    acc.z += cq * x.r0[q].z;
    acc.w += cq * x.r0[q].w;
  }
  for (int j = 4; j < len; j += kRows) {  // kRows rows in flight (same order of the adds: bit-reproducible)
    int oj[kRows];
    float cj[kRows];
    float4 r[kRows];
#pragma unroll
    for (int q = 0; q < kRows; ++q) {
      // contribution min(j + q, 31): lanes >= len hold weight 0 and a valid row; past the chunk: weight 0
      const int jq = min(j + q, ANIREC_CHUNK - 1);
      const int src = kC == 1 ? jq : (jq & (kG - 1)), slot = kC == 1 ? 0 : jq / kG;
      oj[q] = __shfl(pick<kC>(x.o, slot), src, kG);
      cj[q] = j + q < ANIREC_CHUNK ? __shfl(pick<kC>(cf, slot), src, kG) : 0.f;
    }
#pragma unroll
    for (int q = 0; q < kRows; ++q) r[q] = W4[(size_t)oj[q] * kG + l];
#pragma unroll
    for (int q = 0; q < kRows; ++q) {
      acc.x += cj[q] * r[q].x;
      acc.y += cj[q] * r[q].y;
      acc.z += cj[q] * r[q].z;
      acc.w += cj[q] * r[q].w;
    }
  }
  float sfl = sf[0];
#pragma unroll
  for (int k = 1; k < kC; ++k) sfl += sf[k];
  const float ssum = group_sum<kG>(sfl);
  const int gc = T * a.capC + c;  // chunk index inside this parity's P / S
  const size_t pc = (size_t)par * 2 * a.capC + gc;
  reinterpret_cast<float4 *>(a.P)[pc * kG + l] = acc;
  if (l == 0) {
    a.S[pc] = ssum;
    if (rec.w > 0 && a.rowmap != nullptr && rec.x >= a.rowmap_lo)
      a.rowmap[(size_t)par * a.rows + rec.x] = ((gc << 10) | (rec.w - 1)) + 1;
  }
}

template <int kD = kDim>
__device__ __forceinline__ void bwd_body(const BwdArgs &a) {
  constexpr int kG = BwdGeom<kD>::kG;
  // The kernel is a chain of dependent memory round trips at this size, so nothing waits for more than it needs:
  // the step index alone gives the arena slot (chunk record -> sorted index + other-table row -> the rating's
  // scalars and the first four rows are requested at once); both parities' step constants and head partials are
  // requested WITH the step index and the right ones are picked when it has arrived.
  const int step = a.sel[0];
  const StepPub pub0 = a.pub[0], pub1 = a.pub[1];
  // (the partial count of the OTHER parity bounds nothing: rows past a parity's count are never summed)
  BwdMeans h0, h1;
  const int hcap = (int)(a.hpart_stride / kHeadCols);  // partial rows a parity holds
  bwd_means_issue<kG>(a.hpart, hcap, h0);
  bwd_means_issue<kG>(a.hpart + a.hpart_stride, hcap, h1);
  const int par = step & 1;
  BwdPre<BwdGeom<kD>::kC> x;
  bwd_prefetch<kD>(a, step % a.arena_steps, blockIdx.x, x);
  const StepPub pub = par ? pub1 : pub0;
  BwdMeans hm;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int k = (threadIdx.x & (kG - 1)) + kG * q;
    const float2 v = par ? h1.v[q] : h0.v[q];
    hm.v[q] = k < pub.n_head_blocks ? v : make_float2(0.f, 0.f);
  }
  float m[2];
  bwd_means_finish<kG>(a.hpart + par * a.hpart_stride, pub.n_head_blocks, hm, m);
  bwd_chunk<kD>(a, pub, par, m, x);
}

// a row group per chunk, 1024 / kD chunks per workgroup; the occupancy hint and the stamps are 128's alone
template <int kD = kDim>
__global__ __launch_bounds__(256, kD == kDim ? 7 : 1) void k_bwd(BwdArgs a) {
  if constexpr (kD == kDim) tick(a.ticks, 0);
  bwd_body<kD>(a);
  if constexpr (kD == kDim) tick(a.ticks, 1);
}

// g += P[c], s += S[c] for c = c0 .. c1-1 IN THAT ORDER (the sums are bit-reproducible), the loads issued kB
// at a time: a popular anime row has ~30 chunks per batch (one dependent L2 round trip per chunk otherwise)
template <int kB = 8, int kD = kDim>
__device__ __forceinline__ void add_chunks(const float4 *P4, const float *S, int c0, int c1, int l, float4 &g,
                                           float &s) {
  for (int c = c0; c < c1; c += kB) {
    float4 p[kB];
    float sv[kB];
#pragma unroll
    for (int k = 0; k < kB; ++k) {
      const int cc = min(c + k, c1 - 1);
      p[k] = P4[(size_t)cc * (kD / 4) + l];
      sv[k] = S[cc];
    }
#pragma unroll
    for (int k = 0; k < kB; ++k) {
      if (c + k < c1) {
        g.x += p[k].x;
        g.y += p[k].y;
        g.z += p[k].z;
        g.w += p[k].w;
        s += sv[k];
      }
    }
  }
}

// densify part of the gradient for an RCCL collective (multi-GPU): dense[r] = sum of the chunk partials of table
// row dense_lo + r, then dense_rows self-coefficient sums; rows past the table (padding to a multiple of the
// world size for reduce-scatter) are written as zeros.  dense_lo = n_user_rows: the replicated anime table of the
// user-sharded mode; dense_lo = 0: both tables (the literal replicated-table data parallelism).
struct DensifyArgs {
  int dense_lo, n_rows, dense_rows, rows, capC;
  const int32_t *sel;
  int32_t *rowmap;
  const float *P, *S;
  float *dense;
};

__global__ __launch_bounds__(256) void k_densify(DensifyArgs a) {
  const int l = threadIdx.x & 31;
  const int nhw = gridDim.x * 8;
  const int par = a.sel[0] & 1;
  const float4 *P4 = reinterpret_cast<const float4 *>(a.P) + (size_t)par * 2 * a.capC * kRowVec;
  const float *S = a.S + (size_t)par * 2 * a.capC;
  int32_t *rowmap = a.rowmap + (size_t)par * a.rows;
  for (int r = blockIdx.x * 8 + (threadIdx.x >> 5); r < a.dense_rows; r += nhw) {
    const int gr = a.dense_lo + r;
    const int rm = gr < a.n_rows ? rowmap[gr] : 0;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 0.f;
    if (rm) {
      const int first = (rm - 1) >> 10, nch = ((rm - 1) & 1023) + 1;
      add_chunks(P4, S, first, first + nch, l, g, s);
      if (l == 0) rowmap[gr] = 0;
    }
    reinterpret_cast<float4 *>(a.dense)[(size_t)r * kRowVec + l] = g;
    if (l == 0) a.dense[(size_t)a.dense_rows * kDim + r] = s;
  }
}

// ------------------------------------------------------------------------------------
// adam: dense fused update of table rows; the finish of a step (scalar Adam, moving statistics,
// History metrics, cursor) rides in workgroup 0 of the step's last adam launch
// ------------------------------------------------------------------------------------
struct AdamArgs {
  float *W, *M, *V;
  int n_rows;       // this launch covers rows [row_lo, n_rows)
  int row_lo;
  int n_user_rows;  // rows below it count into the user L2 partial, the others into the anime one
  int rows;         // all table rows (stride of the two row maps)
  int capC;
  int parts;        // bit0: write the user-row L2 partials, bit1: the anime-row ones, bit2: finish the step
  int dense_lo, dense_rows;  // dense != nullptr: rows >= dense_lo take their (already reduced) gradient from it
  int32_t *rowmap;  // [2][rows]
  const float *P, *S;
  const float *dense;
  anirec_state *state;
  const StepPub *pub;  // [2]
  const int32_t *sel;
  const float *hpart;
  size_t hpart_stride;
  float two_l2;
  float *regpart;  // [2][2][ANIREC_ADAM_BLOCKS]
  float *ring;         // user-sharded lazy mode: the open window's {n, bce mean} per step (else nullptr; bce = the
                       // loss's data term)
  const int32_t *w0;   // ... and the first step of that window
  unsigned long long *ticks;
};

typedef float f4v __attribute__((ext_vector_type(4)));

// streamed-once data: non-temporal loads/stores keep the three 188-MB streams from thrashing
// L2/MALL lines that the gather kernels of the next step want (measured +6 % on the stream)
__device__ __forceinline__ float4 ld_nt(const float4 *p) {
  const f4v x = __builtin_nontemporal_load(reinterpret_cast<const f4v *>(p));
  return make_float4(x.x, x.y, x.z, x.w);
}
__device__ __forceinline__ void st_nt(float4 *p, const float4 &v) {
  const f4v x = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(x, reinterpret_cast<f4v *>(p));
}
// The same store as ONE opaque instruction: with __builtin_nontemporal_store (or the buffer-descriptor builtin) hipcc
// allocates 160-166 VGPRs for the lazy flush — three waves per SIMD — against 128 with plain stores; the flush wants
// the fourth wave's bytes in flight AND stores that leave the caches to the step kernels.  Nothing ever waits for a
// store, so that hipcc does not count this one in vmcnt costs nothing (cdna_hip_programming.md 5.7: the trailing
// s_nop keeps the next instruction off the data registers until the store has read them).
__device__ __forceinline__ void st_nt_asm(float4 *p, const float4 &v) {
  const f4v x = {v.x, v.y, v.z, v.w};
  asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" : : "v"(p), "v"(x) : "memory");
}

struct RowLoad {
  float4 w, m, v, p0;  // p0: first chunk partial (zero if the row is untouched)
  float s0;
  int rm;              // > 0: chunk list; 0: untouched
};

// issue every load of one row up front: W and the slots the update rule keeps (Adam: M and V; RMSprop / Adagrad: V;
// SGD: none) and — the row map word having been prefetched one iteration earlier — the first chunk partial of a
// touched row
template <bool kNT, int kOpt, int kD = kDim>
__device__ __forceinline__ void row_issue(const AdamArgs &a, int par, int r, int l, int rm, RowLoad &x) {
  constexpr int kG = kD / 4;
  const size_t e = (size_t)r * kG + l;
  x.rm = rm;
  x.p0 = make_float4(0.f, 0.f, 0.f, 0.f);
  x.s0 = 0.f;
  const float4 *Wp = reinterpret_cast<const float4 *>(a.W) + e;
  const float4 *Mp = reinterpret_cast<const float4 *>(a.M) + e;
  const float4 *Vp = reinterpret_cast<const float4 *>(a.V) + e;
  x.w = kNT ? ld_nt(Wp) : *Wp;
  if (kOpt == ANIREC_OPT_ADAM) x.m = kNT ? ld_nt(Mp) : *Mp;
  else x.m = x.p0;  // (zero: not read)
  if (kOpt != ANIREC_OPT_SGD) x.v = kNT ? ld_nt(Vp) : *Vp;
  else x.v = x.p0;
  if (a.dense != nullptr && r >= a.dense_lo) {
    const int dr = r - a.dense_lo;
    x.p0 = reinterpret_cast<const float4 *>(a.dense)[(size_t)dr * kG + l];
    x.s0 = a.dense[(size_t)a.dense_rows * kD + dr];
    x.rm = 0;
  } else if (rm) {
    const size_t first = (size_t)par * 2 * a.capC + ((rm - 1) >> 10);
    x.p0 = reinterpret_cast<const float4 *>(a.P)[first * kG + l];
    x.s0 = a.S[first];
  }
}

// returns sum(W_new^2) of this lane's four elements; the row map word of a touched row is cleared.  `alpha` is the
// step's rate: Adam's bias-corrected alpha, or lr
template <bool kNT, int kOpt, int kB = 4, int kD = kDim>
__device__ __forceinline__ float row_finish(const AdamArgs &a, int par, int r, int l, float alpha, RowLoad &x) {
  constexpr int kG = kD / 4;
  int32_t *rmw = a.rowmap + (size_t)par * a.rows + r;
  const size_t e = (size_t)r * kG + l;
  float4 g = x.p0;
  float s = x.s0;
  if (x.rm) {
    const float4 *P4 = reinterpret_cast<const float4 *>(a.P) + (size_t)par * 2 * a.capC * kG;
    const float *S = a.S + (size_t)par * 2 * a.capC;
    const int first = (x.rm - 1) >> 10, nch = ((x.rm - 1) & 1023) + 1;
    if (nch > 1) add_chunks<kB, kD>(P4, S, first + 1, first + nch, l, g, s);  // rows with > ANIREC_CHUNK contributions
  }
  if (x.rm && l == 0) *rmw = 0;
  float4 w = x.w, m = x.m, v = x.v;
  g.x = grad_total(g.x, s, w.x, a.two_l2);
  g.y = grad_total(g.y, s, w.y, a.two_l2);
  g.z = grad_total(g.z, s, w.z, a.two_l2);
  g.w = grad_total(g.w, s, w.w, a.two_l2);
  opt_elem<kOpt>(w.x, m.x, v.x, g.x, alpha);
  opt_elem<kOpt>(w.y, m.y, v.y, g.y, alpha);
  opt_elem<kOpt>(w.z, m.z, v.z, g.z, alpha);
  opt_elem<kOpt>(w.w, m.w, v.w, g.w, alpha);
  if (kNT) {
    st_nt(reinterpret_cast<float4 *>(a.W) + e, w);
    if (kOpt == ANIREC_OPT_ADAM) st_nt(reinterpret_cast<float4 *>(a.M) + e, m);
    if (kOpt != ANIREC_OPT_SGD) st_nt(reinterpret_cast<float4 *>(a.V) + e, v);
  } else {
    reinterpret_cast<float4 *>(a.W)[e] = w;
    if (kOpt == ANIREC_OPT_ADAM) reinterpret_cast<float4 *>(a.M)[e] = m;
    if (kOpt != ANIREC_OPT_SGD) reinterpret_cast<float4 *>(a.V)[e] = v;
  }
  return w.x * w.x + w.y * w.y + w.z * w.z + w.w * w.w;
}

// block partial of sum(W_new^2): user rows / anime rows, fixed order
__device__ __forceinline__ void block_sq_partials(float sq, float sqa, float *scratch, float *out_u, float *out_a) {
  sq = wave_sum(sq);
  sqa = wave_sum(sqa);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    scratch[threadIdx.x >> 6] = sq;
    scratch[4 + (threadIdx.x >> 6)] = sqa;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (out_u) *out_u = scratch[0] + scratch[1] + scratch[2] + scratch[3];
    if (out_a) *out_a = scratch[4] + scratch[5] + scratch[6] + scratch[7];
  }
  __syncthreads();
}

// the end of step t (one workgroup of 256 threads): reduce the head partials, Adam on (w, b, gamma, beta), moving
// statistics, History sums, cursors.  The L2 term of the loss is sum(W^2) of the weights step t READ: the partials
// the launches of step t-1 (or init_reg) left in the other parity.
// kMode 1 (the lazy dense Adam): the L2 sums of the step are not known yet — the step's batch count and BCE mean go to
// `ring` (slot step - w0) and k_lazy_reduce completes loss / reg_* when the window is flushed.
// kMode 2 (user-sharded multi-GPU step with lazy user rows): the anime table is updated densely every step, so its L2
// sum is here; the user rows' sum is deferred — the step is accounted with the anime term only, its batch count goes
// to `ring`, and k_lazy_reduce adds the user term of every step of the window at the flush.
// kOpt: the update rule of the four scalars (their one slot, if any, is adam_v; the lazy modes are Adam's only).
template <int kMode = 0, int kOpt = ANIREC_OPT_ADAM>
__device__ __forceinline__ void finish_step(const AdamArgs &a, int par, float *scratch, float *ring = nullptr,
                                            int ring_slot = 0) {
  constexpr bool kLazy = kMode == 1;
  const StepPub pub = a.pub[par];
  const float *hpart = a.hpart + par * a.hpart_stride;
  anirec_state *st = a.state;
  // every load of this function is issued before the first use: it is a chain of L2 round trips otherwise
  // (the L2 partials beyond a launch's grid are zero: whole arrays are read, 16 B per lane)
  const int pp = par ^ 1;
  const float4 *ru = reinterpret_cast<const float4 *>(a.regpart + (size_t)(pp * 2 + 0) * ANIREC_ADAM_BLOCKS);
  const float4 *ra = reinterpret_cast<const float4 *>(a.regpart + (size_t)(pp * 2 + 1) * ANIREC_ADAM_BLOCKS);
  float q[2] = {0.f, 0.f};
  if (!kLazy) {
#pragma unroll 2
    for (int i4 = threadIdx.x; i4 < ANIREC_ADAM_BLOCKS / 4; i4 += 256) {
      const float4 v = ra[i4];
      q[1] += (v.x + v.y) + (v.z + v.w);
      if (kMode == 2) continue;  // (the user partials of a lazy-users step are the flush's business)
      const float4 u = ru[i4];
      q[0] += (u.x + u.y) + (u.z + u.w);
    }
  }
  float am[4], av[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    am[k] = st->adam_m[k];
    av[k] = st->adam_v[k];
  }
  const float mmean = st->mov_mean, mvar = st->mov_var;
  const double o_loss = st->loss_wsum, o_bce = st->bce_wsum, o_ru = st->reg_user_wsum, o_ra = st->reg_anime_wsum,
               o_se = st->se_sum, o_n = st->n_seen;
  float h[kHeadCols];
#pragma unroll
  for (int k = 0; k < kHeadCols; ++k) h[k] = 0.f;
  for (int blk = threadIdx.x; blk < pub.n_head_blocks; blk += 256) {
#pragma unroll
    for (int k = 0; k < kHeadCols; ++k) h[k] += hpart[(size_t)blk * kHeadCols + k];
  }
  block_sum<kHeadCols>(h, scratch);
  block_sum<2>(q, scratch);
  if (threadIdx.x == 0) {
    const double n = (double)pub.n_total;
    const double S1 = h[0], S2 = h[1], L = h[2], SE = h[3];
    const double Sdc = h[4], Sc = h[5], Szc = h[6], Sz = h[7];
    const double g = pub.gamma, rs = pub.rs;
    const double m1 = g * S1 / n, m2 = g * S2 / n;
    // sum dz*c and sum dz with dz = (gamma*dy - m1 - zh*m2)*rs, expanded over the batch sums
    // (a batch of one: dz is exactly 0, see bwd_chunk; Sdc is dy * c rounded to fp32 and would leave that rounding)
    const bool one = pub.n_total == 1;
    const float dW = one ? 0.f : (float)(rs * (g * Sdc - m1 * Sc - m2 * Szc));
    const float dB = one ? 0.f : (float)(rs * (g * S1 - n * m1 - m2 * Sz));
    float p4[4] = {pub.w, pub.b, pub.gamma, pub.beta};
    const float g4[4] = {dW, dB, (float)S2, (float)S1};  // d w, d b, d gamma, d beta
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float mm = am[k], vv = av[k];
      opt_elem<kOpt>(p4[k], mm, vv, g4[k], pub.alpha);
      if (kOpt == ANIREC_OPT_ADAM) st->adam_m[k] = mm;
      if (kOpt != ANIREC_OPT_SGD) st->adam_v[k] = vv;
    }
    st->w = p4[0];
    st->b = p4[1];
    st->gamma = p4[2];
    st->beta = p4[3];
    st->mov_mean = mmean - (mmean - pub.mu) * kBnDecay;
    st->mov_var = mvar - (mvar - pub.var) * kBnDecay;
    st->bn_mu = pub.mu;
    st->bn_var = pub.var;
    st->last_mse = (float)(SE / n);
    st->bce_wsum = o_bce + L;
    if (kLazy) {
      ring[2 * ring_slot + 0] = (float)pub.n_total;
      ring[2 * ring_slot + 1] = (float)(L / n);
    } else {
      const float reg_u = q[0], reg_a = q[1];
      const float reg = reg_u + reg_a;
      st->reg_sumsq = reg;
      if (kMode != 2) st->reg_user_sumsq = reg_u;
      st->reg_anime_sumsq = reg_a;
      const float loss = (float)(L / n) + pub.l2 * reg;
      st->last_loss = loss;
      st->loss_wsum = o_loss + (double)loss * n;
      if (kMode != 2) st->reg_user_wsum = o_ru + (double)reg_u * n;
      st->reg_anime_wsum = o_ra + (double)reg_a * n;
      if (kMode == 2) ring[2 * ring_slot + 0] = (float)pub.n_total;
    }
    st->se_sum = o_se + SE;
    st->n_seen = o_n + n;
    st->step_bwd = pub.step;
    st->step_fwd = pub.step + 1;
  }
}

// every row of [row_lo, n_rows) under update rule kOpt (ANIREC_OPT_*); workgroup 0 finishes the step when parts & 4.
// A row is one row group of kD / 4 lanes (a half-wave at 128), 1024 / kD rows per workgroup.
template <bool kNT, int kOpt, int kD = kDim>
__device__ __forceinline__ void adam_body(const AdamArgs &a, int bid, int nblocks, float *scratch) {
  constexpr int kG = kD / 4, kRpb = 256 / kG;
  const int l = threadIdx.x & (kG - 1);
  const int nhw = nblocks * kRpb;
  const int step = a.sel[0];
  const int par = step & 1;
  const float alpha = a.pub[par].alpha;
  const int32_t *rowmap = a.rowmap + (size_t)par * a.rows;
  float sq = 0.f, sqa = 0.f;  // sum(W_new^2) over user rows / anime rows of this thread
  int r = a.row_lo + bid * kRpb + (threadIdx.x / kG);
  // two rows in flight per row group; the row-map words of the NEXT pair are fetched one
  // iteration ahead so a touched row's chunk partial is requested together with W/M/V
  int rm0 = 0, rm1 = 0;
  if (r < a.n_rows) rm0 = rowmap[r];
  if (r + nhw < a.n_rows) rm1 = rowmap[r + nhw];
  for (; r + nhw < a.n_rows; r += 2 * nhw) {
    const int r1 = r + nhw;
    RowLoad x0, x1;
    row_issue<kNT, kOpt, kD>(a, par, r, l, rm0, x0);
    row_issue<kNT, kOpt, kD>(a, par, r1, l, rm1, x1);
    const int rn0 = r + 2 * nhw, rn1 = r + 3 * nhw;
    rm0 = rn0 < a.n_rows ? rowmap[rn0] : 0;
    rm1 = rn1 < a.n_rows ? rowmap[rn1] : 0;
    const float q0 = row_finish<kNT, kOpt, 4, kD>(a, par, r, l, alpha, x0);
    const float q1 = row_finish<kNT, kOpt, 4, kD>(a, par, r1, l, alpha, x1);
    if (r < a.n_user_rows) sq += q0; else sqa += q0;
    if (r1 < a.n_user_rows) sq += q1; else sqa += q1;
  }
  if (r < a.n_rows) {
    RowLoad x0;
    row_issue<kNT, kOpt, kD>(a, par, r, l, rm0, x0);
    const float q0 = row_finish<kNT, kOpt, 4, kD>(a, par, r, l, alpha, x0);
    if (r < a.n_user_rows) sq += q0; else sqa += q0;
  }
  float *rp = a.regpart + (size_t)(par * 2) * ANIREC_ADAM_BLOCKS;
  block_sq_partials(sq, sqa, scratch, (a.parts & 1) ? rp + bid : nullptr,
                    (a.parts & 2) ? rp + ANIREC_ADAM_BLOCKS + bid : nullptr);
  if (bid == 0 && (a.parts & 4)) {
    if (a.ring != nullptr)
      finish_step<2, kOpt>(a, par, scratch, a.ring, step - a.w0[0]);
    else
      finish_step<0, kOpt>(a, par, scratch);
  }
}

// the dense update under any rule (Adam: 24 B/element, SGD: 8, RMSprop / Adagrad: 16) at any width; the stamps are
// taken at 128 only
template <bool kNT, int kOpt = ANIREC_OPT_ADAM, int kD = kDim>
__global__ __launch_bounds__(256) void k_adam(AdamArgs a) {
  __shared__ float scratch[kHeadCols * 16];
  if constexpr (kD == kDim) tick(a.ticks, 0);
  adam_body<kNT, kOpt, kD>(a, blockIdx.x, gridDim.x, scratch);
  if constexpr (kD == kDim) tick(a.ticks, 1);
}

// ------------------------------------------------------------------------------------
// lazy dense Adam (one GPU; include/anirec.h, "LAZY DENSE ADAM")
// ------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_lazy_catchup(LazyArgs a) {
  tick(a.ticks, 0);
  lazy_catchup_row(a, a.state->step_fwd, a.w0[0], blockIdx.x, 0);
  tick(a.ticks, 1);
}

// after bwd(t): step t on the rows the batch touched (chunk gradient - s W + 2 lambda W), the step finish in
// workgroup 0.  Same operations, same order as the dense kernel's row_issue / row_finish for a touched row.
// (the catch-up of batch t + 1's rows rides in k_head(t)'s launch)
// The sparse half walks the anime table's chunk slots first: five workgroups per CU are resident and the user table's
// ~1 250 live workgroups fill them, so behind the user chunks a popular anime row's workgroup — first partial + 8
// rounds of add_chunks<4> for a 31-chunk row, the longest chain of the sparse step — started 3-4 us into the launch.
// Measured, not built: that row's other partials fetched by its whole workgroup in one round trip through LDS.  By
// the per-workgroup stamps (S109M, 8 eager steps) its workgroup ends a launch only when no catch-up rides in it
// (11.3 us against 8.9 for the next one; one step per prepared block); in the launches that carry the next batch's
// catch-up, those workgroups — the last of the grid, started 6.5-8.7 us in — end it at 13-17 us, 2-4 us after the
// 31-chunk row's even where that one started 3.9 us late.
__global__ __launch_bounds__(256) void k_lazy_adam(LazyArgs a, AdamArgs d) {
  __shared__ float scratch[kHeadCols * 16];
  tick(a.ticks, 0);
  const int step = d.sel[0];
  const int par = step & 1;
  const int w0 = a.w0[0];
  const float alpha = d.pub[par].alpha;
  const int l = threadIdx.x & 31;
  if ((int)blockIdx.x >= a.n_sparse) {
    // the slice of the next batch's catch-up that did not ride in head(t)'s launch (see k_head): disjoint rows, no
    // order between it and the sparse step matters
    if (step + 1 < a.n_steps && step + 1 - w0 <= kLzWin)
      lazy_catchup_row(a, step + 1, w0, a.cu_lo + (int)blockIdx.x - a.n_sparse, step + 1);
    tick(a.ticks, 1);
    return;
  }
  int gc, nch;
  const int row = lazy_chunk_row<true>(a, step, (int)blockIdx.x, gc, nch);
  if (row >= 0) {
    const size_t e = (size_t)row * kRowVec + l;
    const float4 *P4 = reinterpret_cast<const float4 *>(d.P) + (size_t)par * 2 * d.capC * kRowVec;
    const float *S = d.S + (size_t)par * 2 * d.capC;
    float4 w = reinterpret_cast<const float4 *>(a.W)[e];
    float4 m = reinterpret_cast<const float4 *>(a.M)[e];
    float4 v = reinterpret_cast<const float4 *>(a.V)[e];
    float4 g = P4[(size_t)gc * kRowVec + l];
    float sc = S[gc];
    if (nch > 1) add_chunks<4>(P4, S, gc + 1, gc + nch, l, g, sc);
    const float sq = halfwave_sum(w.x * w.x + w.y * w.y + w.z * w.z + w.w * w.w);
    g.x = grad_total(g.x, sc, w.x, a.two_l2);
    g.y = grad_total(g.y, sc, w.y, a.two_l2);
    g.z = grad_total(g.z, sc, w.z, a.two_l2);
    g.w = grad_total(g.w, sc, w.w, a.two_l2);
    adam_elem(w.x, m.x, v.x, g.x, alpha);
    adam_elem(w.y, m.y, v.y, g.y, alpha);
    adam_elem(w.z, m.z, v.z, g.z, alpha);
    adam_elem(w.w, m.w, v.w, g.w, alpha);
    reinterpret_cast<float4 *>(a.W)[e] = w;
    reinterpret_cast<float4 *>(a.M)[e] = m;
    reinterpret_cast<float4 *>(a.V)[e] = v;
    if (l == 0) {
      a.z.rowsq[(size_t)row * kLzWin + (step - w0)] = sq;
      a.z.row_step[row] = step + 1;
    }
  }
  if (blockIdx.x == 0 && a.tables == 2) finish_step<1>(d, par, scratch, a.lzring, step - w0);
  tick(a.ticks, 1);
}

// every kLzWin steps and at the end of a run: every row takes its pending steps (one pass over W, M, V for the
// whole window); per step and table the workgroup's sum(W_s^2) — recorded by the earlier kernels for the steps a row
// had already taken, computed here for the replayed ones — goes to lzpart, the sum(W^2) of the weights as they are
// left to the dense path's regpart (both parities: whichever step comes next reads it)
// A workgroup only sees rows of ONE table (workgroups [0, split) stride over the user rows, the others over the anime
// rows): one set of accumulators per thread instead of two.  106 VGPRs: four waves per SIMD, and those — not a row
// prefetched into registers — cover the loads at the top of an iteration (round 3 kept the next row in flight in 12
// more registers at three waves per SIMD: 9 MB in flight chip-wide, a latency-bound 3 TB/s; measured on one box,
// same arithmetic: 262 us with the prefetch at 120 VGPRs, 253 us without).  The stores are non-temporal: with
// plain stores the flush itself is 3 % faster and the step kernels behind it lose more than that (k_bwd +0.8 us,
// k_lazy_reduce +3 us: the flush's dirty lines are what the caches then hold).
template <bool kNT>
__global__ __launch_bounds__(256) void k_lazy_flush(LazyArgs a) {
  __shared__ float red[kLzWin + 1][4];
  tick(a.ticks, 0);
  const int upto = a.state->step_fwd;
  const int w0 = a.w0[0];
  const int nj = upto - w0;
  const int l = threadIdx.x & 31;
  const int tab = (int)blockIdx.x < a.split ? 0 : 1;  // workgroup-uniform
  const int row_lo = tab == 0 ? 0 : a.n_user_rows;
  const int row_hi = tab == 0 ? min(a.n_user_rows, a.lazy_rows) : a.lazy_rows;
  const int nhw = (tab == 0 ? a.split : (int)gridDim.x - a.split) * 8;
  float alpha[kLzWin];
  lazy_alphas(a, w0, nj, alpha);
  const LzBound bd = lz_bound(alpha, nj, a.two_l2);
  float acc[kLzWin];
#pragma unroll
  for (int j = 0; j < kLzWin; ++j) acc[j] = 0.f;
  float fin = 0.f;
  auto load_row = [&](int r, Row3 &x) {
    const size_t e = (size_t)r * kRowVec + l;
    const float4 *Wp = reinterpret_cast<const float4 *>(a.W) + e, *Mp = reinterpret_cast<const float4 *>(a.M) + e,
                 *Vp = reinterpret_cast<const float4 *>(a.V) + e;
    x.w = kNT ? ld_nt(Wp) : *Wp;
    x.m = kNT ? ld_nt(Mp) : *Mp;
    x.v = kNT ? ld_nt(Vp) : *Vp;
  };
  for (int r = row_lo + ((int)blockIdx.x - (tab == 0 ? 0 : a.split)) * 8 + (threadIdx.x >> 5); r < row_hi; r += nhw) {
    Row3 x;
    const int ta = a.z.row_step[r];
    load_row(r, x);
    const int jt = ta - w0;  // steps [0, jt) of the window are on record, [jt, nj) are pending
    const size_t e = (size_t)r * kRowVec + l;
    float rec = 0.f;
    if (l < jt) rec = a.z.rowsq[(size_t)r * kLzWin + l];  // lane j holds the recorded sum of step j
    // sq[j]: lane j's recorded row sum of step j (rec is 0 on lanes l >= jt), overwritten for the replayed steps
    // [jt, nj) by their lane parts — what the accumulators take, with no select-and-add per step
    float sq[kLzWin];
#pragma unroll
    for (int j = 0; j < kLzWin; ++j) sq[j] = l == j ? rec : 0.f;
    if (jt < nj) {
      lazy_replay<true>(x, jt, nj, alpha, a.two_l2, bd, sq, a.W, a.M, a.V, e);
      if (kNT) {
        st_nt_asm(reinterpret_cast<float4 *>(a.W) + e, x.w);
        st_nt_asm(reinterpret_cast<float4 *>(a.M) + e, x.m);
        st_nt_asm(reinterpret_cast<float4 *>(a.V) + e, x.v);
      } else {
        reinterpret_cast<float4 *>(a.W)[e] = x.w;
        reinterpret_cast<float4 *>(a.M)[e] = x.m;
        reinterpret_cast<float4 *>(a.V)[e] = x.v;
      }
      if (l == 0) a.z.row_step[r] = upto;
    }
#pragma unroll
    for (int j = 0; j < kLzWin; ++j) acc[j] += sq[j];
    fin += x.w.x * x.w.x + x.w.y * x.w.y + x.w.z * x.w.z + x.w.w * x.w.w;
  }
  // block sums in a fixed order: lanes -> waves -> the four waves
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < kLzWin; ++j) {
    const float v = wave_sum(acc[j]);
    if ((threadIdx.x & 63) == 0) red[j][wv] = v;
  }
  {
    const float v = wave_sum(fin);
    if ((threadIdx.x & 63) == 0) red[kLzWin][wv] = v;
  }
  __syncthreads();
  if (threadIdx.x <= kLzWin) {
    const int j = threadIdx.x;
    const float v = ((red[j][0] + red[j][1]) + red[j][2]) + red[j][3];
    if (j < kLzWin) {  // the other table's slot of this workgroup is zero by definition
      a.lzpart[((size_t)j * 2 + tab) * ANIREC_ADAM_BLOCKS + blockIdx.x] = v;
      a.lzpart[((size_t)j * 2 + (tab ^ 1)) * ANIREC_ADAM_BLOCKS + blockIdx.x] = 0.f;
    } else {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (t < a.tables) {  // (tables == 1: the anime partials belong to the dense launches of every step)
          const float u = t == tab ? v : 0.f;
          a.regpart[(size_t)(0 * 2 + t) * ANIREC_ADAM_BLOCKS + blockIdx.x] = u;
          a.regpart[(size_t)(1 * 2 + t) * ANIREC_ADAM_BLOCKS + blockIdx.x] = u;
        }
      }
    }
  }
  tick(a.ticks, 1);
}

// (Measured and not built: the window's flush on a side stream beside the NEXT window's steps — emulated with a
// flush that replays every row regardless of state, 1 / 2 / 4 / 8 / 32 workgroups per CU, timing only: 0.095 / 0.100 /
// 0.100 / 0.102 / 0.103 ms per step against 0.101 — the latency-bound step kernels lose beside the VALU-bound flush
// what the flush gains beside them.)
// one workgroup of 16 waves: wave (2 j + table) sums the flush's block partials of step j in a fixed order, then
// one thread completes the History sums of the window's steps in step order and opens the next window
__global__ __launch_bounds__(1024) void k_lazy_reduce(LazyArgs a) {
  __shared__ float reg[kLzWin][2];
  tick(a.ticks, 0);
  const int upto = a.state->step_fwd;
  const int w0 = a.w0[0];
  const int nj = upto - w0;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  static_assert(2 * kLzWin <= 16, "one wave per (step, table)");
  if (wv < 2 * kLzWin) {
    // wv = 2 j + table; 32 x 16 B per lane, every load issued before the first add (a dependent scalar loop
    // measured 38 us for this workgroup)
    const float4 *p = reinterpret_cast<const float4 *>(a.lzpart + (size_t)wv * ANIREC_ADAM_BLOCKS);
    constexpr int kV = ANIREC_ADAM_BLOCKS / 4 / 64;
    float4 v[kV];
#pragma unroll
    for (int i = 0; i < kV; ++i) v[i] = p[lane + 64 * i];
    float sacc = 0.f;
#pragma unroll
    for (int i = 0; i < kV; ++i) sacc += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    sacc = wave_sum(sacc);
    if (lane == 0) reg[wv >> 1][wv & 1] = sacc;
  }
  __syncthreads();
  if (threadIdx.x == 0 && nj > 0) {
    anirec_state *st = a.state;
    double o_loss = st->loss_wsum, o_ru = st->reg_user_wsum, o_ra = st->reg_anime_wsum;
    float loss = 0.f, ru = 0.f, ra = 0.f;
    if (a.tables == 1) {
      // user rows only: every step of the window was accounted with its anime term when it finished; add the user
      // term (this rank's rows) of each
      for (int j = 0; j < nj && j < kLzWin; ++j) {
        const double n = (double)a.lzring[2 * j + 0];
        ru = reg[j][0];
        o_loss += (double)(a.l2 * ru) * n;
        o_ru += (double)ru * n;
      }
      st->loss_wsum = o_loss;
      st->reg_user_wsum = o_ru;
      st->last_loss = st->last_loss + a.l2 * ru;
      st->reg_user_sumsq = ru;
      st->reg_sumsq = ru + st->reg_anime_sumsq;
    } else {
      for (int j = 0; j < nj && j < kLzWin; ++j) {
        const double n = (double)a.lzring[2 * j + 0];
        ru = reg[j][0];
        ra = reg[j][1];
        loss = a.lzring[2 * j + 1] + a.l2 * (ru + ra);
        o_loss += (double)loss * n;
        o_ru += (double)ru * n;
        o_ra += (double)ra * n;
      }
      st->loss_wsum = o_loss;
      st->reg_user_wsum = o_ru;
      st->reg_anime_wsum = o_ra;
      st->last_loss = loss;
      st->reg_sumsq = ru + ra;
      st->reg_user_sumsq = ru;
      st->reg_anime_sumsq = ra;
    }
    a.w0[0] = upto;
  }
  tick(a.ticks, 1);
}

// sum(W^2) partials of the CURRENT weights into both parities (after (re)loading weights, before validation):
// the next step's finish reads them whatever its parity
template <int kD = kDim>
__device__ __forceinline__ void reg_init_body(const float *W, int row_lo, int n_rows, int n_user_rows,
                                              float *regpart) {
  __shared__ float scratch[16];
  __shared__ float res[2];
  constexpr int kG = kD / 4, kRpb = 256 / kG;
  const int l = threadIdx.x & (kG - 1);
  const int nhw = gridDim.x * kRpb;
  float sq = 0.f, sqa = 0.f;
  for (int r = row_lo + blockIdx.x * kRpb + (threadIdx.x / kG); r < n_rows; r += nhw) {
    const float4 w = reinterpret_cast<const float4 *>(W)[(size_t)r * kG + l];
    const float q = w.x * w.x + w.y * w.y + w.z * w.z + w.w * w.w;
    if (r < n_user_rows) sq += q; else sqa += q;
  }
  block_sq_partials(sq, sqa, scratch, &res[0], &res[1]);
  const float u = res[0], an = res[1];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      regpart[(size_t)(p * 2 + 0) * ANIREC_ADAM_BLOCKS + blockIdx.x] = u;
      regpart[(size_t)(p * 2 + 1) * ANIREC_ADAM_BLOCKS + blockIdx.x] = an;
    }
  }
}
template <int kD = kDim>
__global__ __launch_bounds__(256) void k_reg_init(const float *W, int row_lo, int n_rows, int n_user_rows,
                                                  float *regpart) {
  reg_init_body<kD>(W, row_lo, n_rows, n_user_rows, regpart);
}

__global__ __launch_bounds__(1024) void k_sum_regpart(anirec_state *st, const float *regpart) {
  __shared__ float scratch[2 * 16];
  float r[2] = {0.f, 0.f};
  for (int i = threadIdx.x; i < 2 * ANIREC_ADAM_BLOCKS / 4; i += blockDim.x) {
    const float4 v = reinterpret_cast<const float4 *>(regpart)[i];
    r[i >= ANIREC_ADAM_BLOCKS / 4 ? 1 : 0] += (v.x + v.y) + (v.z + v.w);
  }
  block_sum<2>(r, scratch);
  if (threadIdx.x == 0) {
    st->reg_user_sumsq = r[0];
    st->reg_anime_sumsq = r[1];
    st->reg_sumsq = r[0] + r[1];
  }
}

// Self-test of the whole replay on given rows (anirec_selftest_lazy_replay; tests only): one half-wave per row takes
// the row's pending steps [j0[row], nj) by lazy_replay with the flush's once-per-row test (row_test) or the
// catch-up's per-step one — the packed sequences, the row test, the redo by the
// compiler's expansions — and, separately, by the dense kernel's adam_elem; fast[row] = 1 if every lane of the row
// passed the short sequences' range test (the row alone would not trigger the redo).  wmv / out_*: [3][rows][kDim].
// (It is here, beside the lazy kernels, and not with the other two self-tests in anirec_train_util.hip: it never reads
// the sq[] that lazy_replay_slow returns, and in a unit where it is the only caller the compiler cuts that part out of
// the unit's copy of the function.  Here it runs the very copy the lazy kernels run.)
__global__ __launch_bounds__(256) void k_selftest_lazy_replay(const float *wmv, int rows, const float *alpha8, int nj,
                                                              const int32_t *j0s, float two_l2, float *out_lazy,
                                                              float *out_dense, int32_t *fast, int row_test) {
  const int row = (int)blockIdx.x * 8 + (int)(threadIdx.x >> 5);
  const int l = threadIdx.x & 31;
  if (row >= rows) return;
  const size_t plane = (size_t)rows * kRowVec;
  const size_t e = (size_t)row * kRowVec + l;
  const float *W = wmv, *M = wmv + plane * 4, *V = wmv + plane * 8;
  Row3 x;
  x.w = reinterpret_cast<const float4 *>(W)[e];
  x.m = reinterpret_cast<const float4 *>(M)[e];
  x.v = reinterpret_cast<const float4 *>(V)[e];
  const Row3 x0 = x;
  float alpha[kLzWin], sq[kLzWin];
#pragma unroll
  for (int j = 0; j < kLzWin; ++j) {
    alpha[j] = j < nj ? alpha8[j] : 0.f;
    sq[j] = 0.f;
  }
  const LzBound bd = lz_bound(alpha, nj, two_l2);
  const int j0 = j0s[row];
  {
    Row3 t = x;
    float sqt[kLzWin];
    const bool ok = row_test ? lazy_replay_path<true, true>(t, j0, nj, alpha, two_l2, bd, sqt)
                             : lazy_replay_path<true, false>(t, j0, nj, alpha, two_l2, bd, sqt);
    const unsigned long long badm = __ballot(!ok);
    if (l == 0) fast[row] = ((badm >> (threadIdx.x & 32)) & 0xFFFFFFFFull) == 0 ? 1 : 0;
  }
  if (row_test)
    lazy_replay<true>(x, j0, nj, alpha, two_l2, bd, sq, W, M, V, e);
  else
    lazy_replay<false>(x, j0, nj, alpha, two_l2, bd, sq, W, M, V, e);
  float4 *o = reinterpret_cast<float4 *>(out_lazy);
  o[e] = x.w;
  o[plane + e] = x.m;
  o[2 * plane + e] = x.v;
  Row3 y = x0;
  for (int j = j0 < 0 ? 0 : j0; j < nj; ++j) {
    float q;
    LzRange unused{};
    lazy_one_step<false, false>(y, alpha[j], two_l2, q, unused);
  }
  float4 *od = reinterpret_cast<float4 *>(out_dense);
  od[e] = y.w;
  od[plane + e] = y.m;
  od[2 * plane + e] = y.v;
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------
static inline float *packet_ptr(const anirec_train_desc *d, int seg) {
  return d->packets + anirec_packet_floats(d->max_batch) * (size_t)seg;
}

// measurement hook armed (anirec_train_stage_ticks): kernels stamp their workgroups' start / end times
bool g_ticks_on = false;
static double g_tick_sum_us[8];  // per kernel: sum of the launch durations since the hook was last read
static int g_tick_launches[8];
// armed only: wait for the launch just made, turn its workgroups' stamps into ONE duration (max end - min start),
// add it to the kernel's sum and clear the slot for the next launch
int ticks_collect(const TrainWs &w, int kernel, hipStream_t s) {
  if (!g_ticks_on) return ANIREC_OK;
  static unsigned long long h[2 * ANIREC_ADAM_BLOCKS];
  unsigned long long *dev = w.ticks + (size_t)kernel * 2 * ANIREC_ADAM_BLOCKS;
  ANIREC_HIP_CHECK(hipStreamSynchronize(s));
  ANIREC_HIP_CHECK(hipMemcpy(h, dev, sizeof(h), hipMemcpyDeviceToHost));
  unsigned long long lo = ~0ull, hi = 0ull;
  for (int b = 0; b < ANIREC_ADAM_BLOCKS; ++b) {
    if (h[2 * b] != 0ull && h[2 * b] < lo) lo = h[2 * b];
    if (h[2 * b + 1] > hi) hi = h[2 * b + 1];
  }
  if (hi > 0ull && lo != ~0ull && hi >= lo) {
    g_tick_sum_us[kernel] += (double)(hi - lo) * 0.01;
    g_tick_launches[kernel] += 1;
  }
  ANIREC_HIP_CHECK(hipMemsetAsync(dev, 0, sizeof(h), s));
  return ANIREC_OK;
}

static FwdArgs fwd_args(const anirec_train_desc *d, const TrainWs &w) {
  FwdArgs a;
  a.W = d->W;
  a.n_user_rows = d->n_user_rows;
  a.user_idx = d->user_idx;
  a.anime_idx = d->anime_idx;
  a.rating = d->rating;
  a.sched = d->sched;
  a.state = d->state;
  float *pk = packet_ptr(d, d->my_seg);
  a.pk_c = pk;
  a.pk_t = pk + packet_cap(d->max_batch);
  a.pk_count = reinterpret_cast<int32_t *>(pk + 2 * (size_t)packet_cap(d->max_batch));
  a.su = w.su;
  a.sa = w.sa;
  a.cap = d->max_batch;
  a.touched = (d->lazy != 0 && d->lazy_state != nullptr && d->dense_mode != 2)
                  ? lazy_carve(d->lazy_state, table_rows(d)).mark
                  : nullptr;
  a.ticks = ticks_of(w, 0);
  return a;
}

int launch_fwd(const anirec_train_desc *d, const TrainWs &w, hipStream_t s) {
  const FwdArgs a = fwd_args(d, w);
  float *pk = packet_ptr(d, d->my_seg);
  with_width(w.dim, [&](auto kd) {
    constexpr int kD = decltype(kd)::value, kRpb = 1024 / kD;
    hipLaunchKernelGGL(k_fwd<kD>, dim3((d->max_batch + kRpb - 1) / kRpb), dim3(256), 0, s, a);
  });
  if (int te = ticks_collect(w, 0, s)) return te;
  if (d->n_seg > 1)
    hipLaunchKernelGGL(k_seg_stats, dim3(1), dim3(1024), 0, s, pk, packet_cap(d->max_batch), d->max_batch,
                       d->state);
  return (int)hipGetLastError();
}

int launch_densify(const anirec_train_desc *d, const TrainWs &w, hipStream_t s) {
  DensifyArgs g;
  g.dense_lo = dense_lo_of(d);
  g.n_rows = table_rows(d);
  g.dense_rows = d->dense_rows;
  g.rows = table_rows(d);
  g.capC = w.capC;
  g.sel = w.sel;
  g.rowmap = d->rowmap;
  g.P = w.P;
  g.S = w.S;
  g.dense = d->dense_grad;
  int blocks = (d->dense_rows + 7) / 8;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_densify, dim3(blocks), dim3(256), 0, s, g);
  return (int)hipGetLastError();
}

// bwd only (the densify pass of the multi-GPU modes is a separate launch so that the caller can fork work
// that needs the chunk partials but not the dense buffer)
static BwdArgs bwd_args(const anirec_train_desc *d, const TrainWs &w) {
  BwdArgs a;
  a.W = d->W;
  a.pub = w.pub;
  a.sel = w.sel;
  a.hpart = w.hpart;
  a.hpart_stride = w.hpart_stride;
  a.rows = table_rows(d);
  a.arena = w.arena;
  a.slot_bytes = w.slot_bytes;
  a.cap = w.cap;
  a.capC = w.capC;
  a.pk_c = packet_ptr(d, d->my_seg);
  a.dy = w.dy;
  a.su = w.su;
  a.sa = w.sa;
  a.P = w.P;
  a.S = w.S;
  a.rowmap = d->rowmap;
  a.rowmap_lo = 0;
  a.arena_steps = w.arena_steps;
  a.ticks = ticks_of(w, 2);
  return a;
}

int launch_bwd_only(const anirec_train_desc *d, const TrainWs &w, hipStream_t s, bool lazy) {
  BwdArgs a = bwd_args(d, w);
  if (lazy) {  // the lazy update walks the chunk table itself: no row map to fill (or to clear)
    if (d->dense_mode == 1)
      a.rowmap_lo = d->n_user_rows;  // (user-sharded step: the densify pass still wants the anime rows' words)
    else
      a.rowmap = nullptr;
  }
  with_width(w.dim, [&](auto kd) {
    constexpr int kD = decltype(kd)::value, kRpb = BwdGeom<kD>::kRpb;
    hipLaunchKernelGGL(k_bwd<kD>, dim3((2 * w.capC + kRpb - 1) / kRpb), dim3(256), 0, s, a);
  });
  if (int te = ticks_collect(w, 2, s)) return te;
  return (int)hipGetLastError();
}

int launch_bwd(const anirec_train_desc *d, const TrainWs &w, hipStream_t s) {
  int e = launch_bwd_only(d, w, s);
  if (!e && d->dense_mode) e = launch_densify(d, w, s);
  return e;
}

// Grid of a launch that streams `rows` table rows (the dense updates and the L2 init: the whole table; the lazy flush:
// the lazily updated rows): a function of the row count only, so the same regpart / partial slots are rewritten each
// launch.  Two rows per half-wave at least, so the two-rows-in-flight pipeline has something to overlap on small
// (cache-resident) tables.
static inline int stream_grid(long long rows) {
  long long b = (rows + 15) / 16;
  if (b < 64) b = 64;
  if (b > ANIREC_ADAM_BLOCKS) b = ANIREC_ADAM_BLOCKS;
  return (int)b;
}

static AdamArgs adam_args(const anirec_train_desc *d, const TrainWs &w) {
  AdamArgs a;
  a.W = d->W;
  a.M = d->M;
  a.V = d->V;
  a.n_rows = table_rows(d);
  a.row_lo = 0;
  a.n_user_rows = d->n_user_rows;
  a.rows = table_rows(d);
  a.capC = w.capC;
  a.parts = 7;
  a.dense_lo = dense_lo_of(d);
  a.dense_rows = d->dense_rows;
  a.rowmap = d->rowmap;
  a.P = w.P;
  a.S = w.S;
  a.dense = d->dense_mode ? d->dense_grad : nullptr;
  a.state = d->state;
  a.pub = w.pub;
  a.sel = w.sel;
  a.hpart = w.hpart;
  a.hpart_stride = w.hpart_stride;
  a.two_l2 = 2.0f * d->l2;
  a.regpart = w.regpart;
  a.ring = nullptr;
  a.w0 = nullptr;
  a.ticks = ticks_of(w, 3);
  return a;
}

// tables that overflow the 256-MiB Infinity Cache are streamed non-temporally; small ones
// (the 7M-rating shape: 50 MB of W+M+V) stay cache-resident between steps
static inline bool stream_nt(const anirec_train_desc *d, int dim = kDim) {
  return (size_t)table_rows(d) * dim * 4 * 3 > ((size_t)192 << 20);
}
// grid of the dense update and of the L2 init (the same: both write the regpart slots [0, grid)): sized by the tables'
// bytes, so a row group has two rows at least at every width
static inline int table_grid(const anirec_train_desc *d, const TrainWs &w) {
  return stream_grid((long long)table_rows(d) * w.dim / kDim);
}

// which: 0 = every row this rank updates + finish (one GPU; replicated multi-GPU modes), 1 = the user rows only (may
// run while the anime gradient is still in the all-reduce: user-sharded mode), 2 = the anime rows + finish
int launch_adam_full(const anirec_train_desc *d, const TrainWs &w, hipStream_t s, int which) {
  AdamArgs a = adam_args(d, w);
  if (d->dense_mode == 2 && (d->adam_row_lo | d->adam_row_hi)) {  // reduce-scatter shard (possibly empty)
    a.row_lo = d->adam_row_lo;
    a.n_rows = d->adam_row_hi;
  }
  if (which == 1) {
    a.n_rows = d->n_user_rows;
    a.parts = 1;
  } else if (which == 2) {
    a.row_lo = d->n_user_rows;
    a.parts = 2 | 4;
    if (lazy_users(d)) {  // the step is accounted with its anime L2 term only; the flush adds the user rows' (finish_step<2>)
      a.ring = w.lzring;
      a.w0 = w.sel + 1;
    }
  }
  const bool nt = stream_nt(d, w.dim);
  const dim3 grid(table_grid(d, w)), block(256);
  with_width(w.dim, [&](auto kd) {  // (off 128: the dense one-GPU step only, check_desc)
    with_opt(d->optimizer, [&](auto opt) {
      constexpr int kD = decltype(kd)::value, kOpt = decltype(opt)::value;
      if (nt) hipLaunchKernelGGL((k_adam<true, kOpt, kD>), grid, block, 0, s, a);
      else hipLaunchKernelGGL((k_adam<false, kOpt, kD>), grid, block, 0, s, a);
    });
  });
  if (int te = ticks_collect(w, 3, s)) return te;
  return (int)hipGetLastError();
}

// ---- lazy dense Adam: host side ----
LazyArgs lazy_args(const anirec_train_desc *d, const TrainWs &w, int ticks_slot) {
  LazyArgs a;
  a.W = d->W;
  a.M = d->M;
  a.V = d->V;
  a.rows = table_rows(d);
  a.n_user_rows = d->n_user_rows;
  a.z = lazy_carve(d->lazy_state, table_rows(d));
  a.sched = d->sched;
  a.n_steps = d->n_steps;
  a.state = d->state;
  a.w0 = w.sel + 1;
  a.two_l2 = 2.0f * d->l2;
  a.l2 = d->l2;
  a.arena = w.arena;
  a.slot_bytes = w.slot_bytes;
  a.cap = w.cap;
  a.capC = w.capC;
  a.arena_steps = w.arena_steps;
  a.lzpart = w.lzpart;
  a.lzring = w.lzring;
  a.regpart = w.regpart;
  a.tables = lazy_users(d) ? 1 : 2;
  a.lazy_rows = lazy_users(d) ? d->n_user_rows : table_rows(d);
  a.split = 0;
  a.cu_lo = 0;
  a.n_sparse = 0x7fffffff;
  a.ticks = ticks_of(w, ticks_slot);
  return a;
}

// every row is current as of `first_step` (every run ends flushed): open a window there
int lazy_begin(const anirec_train_desc *d, const TrainWs &w, int first_step, hipStream_t s) {
  const LazyState z = lazy_carve(d->lazy_state, table_rows(d));
  ANIREC_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)z.row_step, first_step, (size_t)table_rows(d), s));
  ANIREC_HIP_CHECK(hipMemsetAsync(z.mark, 0, sizeof(int32_t) * (size_t)table_rows(d), s));  // (marks of an earlier schedule)
  ANIREC_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)(w.sel + 1), first_step, 1, s));
  return ANIREC_OK;
}

int launch_lazy_catchup(const anirec_train_desc *d, const TrainWs &w, hipStream_t s) {
  hipLaunchKernelGGL(k_lazy_catchup, dim3(lazy_chunk_grid(d, w)), dim3(256), 0, s, lazy_args(d, w, 4));
  if (int e = ticks_collect(w, 4, s)) return e;
  return (int)hipGetLastError();
}

// the sparse step of the batch bwd has just processed
int launch_lazy_adam(const anirec_train_desc *d, const TrainWs &w, hipStream_t s, bool fuse_next) {
  const int grid = lazy_chunk_grid(d, w);
  AdamArgs aa = adam_args(d, w);
  aa.ticks = nullptr;
  LazyArgs la = lazy_args(d, w, 5);
  la.n_sparse = grid;
  la.cu_lo = catchup_head_share(d, w);
  const int extra = fuse_next ? grid - la.cu_lo : 0;
  hipLaunchKernelGGL(k_lazy_adam, dim3(grid + extra), dim3(256), 0, s, la, aa);
  if (int e = ticks_collect(w, 5, s)) return e;
  return (int)hipGetLastError();
}

int lazy_flush(const anirec_train_desc *d, const TrainWs &w, hipStream_t s) {
  LazyArgs a = lazy_args(d, w, 6);
  const int grid = stream_grid(a.lazy_rows);
  // the grid's share of each table (a function of the table sizes only: the same partial slots every window)
  a.split = grid;
  if (a.tables == 2) {
    long long sp = ((long long)grid * d->n_user_rows + table_rows(d) / 2) / table_rows(d);
    if (sp < 1) sp = 1;
    if (sp > grid - 1) sp = grid - 1;
    a.split = (int)sp;
  }
  if (stream_nt(d))
    hipLaunchKernelGGL((k_lazy_flush<true>), dim3(grid), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((k_lazy_flush<false>), dim3(grid), dim3(256), 0, s, a);
  if (int te = ticks_collect(w, 6, s)) return te;
  hipLaunchKernelGGL(k_lazy_reduce, dim3(1), dim3(1024), 0, s, lazy_args(d, w, 7));
  if (int te = ticks_collect(w, 7, s)) return te;
  return (int)hipGetLastError();
}

int launch_prep(const anirec_train_desc *d, const TrainWs &w, int first_step, int n_steps,
                       bool relative_to_cursor, hipStream_t s) {
  PrepArgs a;
  a.user_idx = d->user_idx;
  a.anime_idx = d->anime_idx;
  a.sched = d->sched;
  a.first_step = first_step;
  a.cursor = relative_to_cursor ? d->state : nullptr;
  a.n_steps_total = d->n_steps;
  a.n_user_rows = d->n_user_rows;
  a.n_anime_rows = d->n_anime_rows;
  a.cap = w.cap;
  a.capC = w.capC;
  a.arena_steps = w.arena_steps;
  a.arena = w.arena;
  a.slot_bytes = w.slot_bytes;
  hipLaunchKernelGGL(k_prep, dim3(2 * n_steps), dim3(kSortThreads), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace anirec

using namespace anirec;

extern "C" {

int anirec_train_init_reg_w(const anirec_train_desc *d, int32_t dim, void *stream) {
  int rc = check_desc(d, dim);
  if (rc) return rc;
  TrainWs w = carve(d->workspace, d->max_batch, d->arena_steps, dim);
  hipStream_t s = (hipStream_t)stream;
  // entries beyond the grid are never written again: they must be (and stay) zero
  ANIREC_HIP_CHECK(hipMemsetAsync(w.regpart, 0, sizeof(float) * 4 * ANIREC_ADAM_BLOCKS, s));
  // a rank that only updates a row shard (replicated tables + reduce-scatter) only counts that shard, like its
  // adam launches do: the caller sums the ranks' values
  int lo = 0, hi = table_rows(d);
  if (d->dense_mode == 2 && (d->adam_row_lo | d->adam_row_hi)) {
    lo = d->adam_row_lo;
    hi = d->adam_row_hi;
  }
  const dim3 grid(table_grid(d, w));
  with_width(dim, [&](auto kd) {
    hipLaunchKernelGGL(k_reg_init<decltype(kd)::value>, grid, dim3(256), 0, s, d->W, lo, hi, d->n_user_rows, w.regpart);
  });
  ANIREC_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_sum_regpart, dim3(1), dim3(1024), 0, s, d->state, w.regpart);
  return (int)hipGetLastError();
}
int anirec_train_init_reg(const anirec_train_desc *d, void *stream) {
  return anirec_train_init_reg_w(d, ANIREC_DIM, stream);
}

// Measurement hook (bench.py).  While armed, every training kernel launched through this library stamps the
// constant-clock (100 MHz) time of each workgroup's first and last instruction into the workspace, and the launch
// function waits for it and adds max(end) - min(start) over its workgroups to the kernel's sum.  This call returns,
// per kernel (0 fwd, 1 head, 2 bwd, 3 adam, 4 lazy catch-up, 5 lazy adam, 6 lazy flush, 7 lazy reduce), the MEAN
// duration [us] of the launches made since the last call (-1 = none) and their number, then arms (enable != 0) or
// disarms.  Armed steps run eagerly (never from the captured graph) and synchronise after every launch.
int anirec_train_stage_ticks(const anirec_train_desc *d, int32_t enable, float *us8_host, int32_t *launches8_host,
                             void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  TrainWs w = carve(d->workspace, d->max_batch, d->arena_steps);
  for (int k = 0; k < 8; ++k) {
    if (us8_host) us8_host[k] = g_tick_launches[k] ? (float)(g_tick_sum_us[k] / g_tick_launches[k]) : -1.0f;
    if (launches8_host) launches8_host[k] = g_tick_launches[k];
    g_tick_sum_us[k] = 0.0;
    g_tick_launches[k] = 0;
  }
  ANIREC_HIP_CHECK(hipStreamSynchronize(s));
  ANIREC_HIP_CHECK(hipMemsetAsync(w.ticks, 0, sizeof(unsigned long long) * 8 * 2 * ANIREC_ADAM_BLOCKS, s));
  g_ticks_on = enable != 0;
  return ANIREC_OK;
}

int anirec_selftest_lazy_replay(const float *wmv, int32_t rows, const float *alpha8, int32_t nj, const int32_t *j0,
                                float two_l2, int32_t row_test, float *out_lazy, float *out_dense, int32_t *fast,
                                void *stream) {
  if (!wmv || !alpha8 || !j0 || !out_lazy || !out_dense || !fast || rows <= 0 || nj < 0 || nj > ANIREC_LAZY_WINDOW)
    return ANIREC_EINVAL;
  hipLaunchKernelGGL(k_selftest_lazy_replay, dim3((unsigned)((rows + 7) / 8)), dim3(256), 0, (hipStream_t)stream,
                     wmv, (int)rows, alpha8, (int)nj, j0, two_l2, out_lazy, out_dense, fast, (int)(row_test != 0));
  return (int)hipGetLastError();
}

}  // extern "C"
