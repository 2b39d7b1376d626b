// The output head's device code, inlined into the kernels of three units: k_head (anirec_train_head.hip),
// k_head_metrics (anirec_train_head_metrics.hip) and the validation kernels (anirec_train_eval.hip, the metrics only).
#pragma once
#include "anirec_train.hpp"

namespace anirec {

// ------------------------------------------------------------------------------------
// head: Dense(1) -> BatchNorm(batch stats) -> activation -> loss (head_terms), spread over many workgroups.
// Every workgroup recomputes the batch mean/variance of z from all c (two-pass, no
// transcendentals, 40 KB from L2), then does the sigmoid/log work of ITS 256 ratings and
// leaves eight partial sums.  Workgroup 0 publishes the step constants for bwd / adam.
// ------------------------------------------------------------------------------------

// the packet count word travels through an all-gather on the multi-GPU path: read it with an agent-scope load
__device__ __forceinline__ int ld_i32(const int32_t *p) {
  return __hip_atomic_load(const_cast<int32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int packet_count(const float *pk, int cap) {
  return min(ld_i32(reinterpret_cast<const int32_t *>(pk + 2 * (size_t)packet_cap(cap))), cap);
}

// A packet's c values for the batch statistics: every 16-B load of the thread is issued before
// the first use (a scalar strided loop serialises ~40 L2 round trips) and does not depend on
// the packet's count word, so state, counts and values arrive in ONE memory round trip.
constexpr int kHeadVec = ANIREC_MAX_BATCH / (4 * kHeadThreads);  // 16 float4 per thread at most

// A packet's c values for the batch statistics: every 16-B load of the thread is issued before the first use (a
// scalar strided loop serialises ~40 L2 round trips) and does not depend on the packet's count word, so state,
// counts and values arrive in ONE memory round trip; they stay in registers for both passes (re-reading them
// from L2 for the second pass measured 12.1 us per launch against 8.8 us).
struct SegVals {
  float4 v[kHeadVec];
};

__device__ __forceinline__ void seg_load(const float *pk, int pcap, SegVals &x) {
  const float4 *p4 = reinterpret_cast<const float4 *>(pk);
#pragma unroll
  for (int k = 0; k < kHeadVec; ++k) {
    const int i4 = threadIdx.x + k * kHeadThreads;
    x.v[k] = (i4 * 4 < pcap) ? p4[i4] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

template <bool kSecond>
__device__ __forceinline__ float seg_stat(const SegVals &x, int cnt, float w, float b, float mu) {
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < kHeadVec; ++k) {
    const int i = (threadIdx.x + k * kHeadThreads) * 4;
    const float c4[4] = {x.v[k].x, x.v[k].y, x.v[k].z, x.v[k].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i + j < cnt) {
        const float z = c4[j] * w + b;
        acc += kSecond ? (z - mu) * (z - mu) : z;
      }
    }
  }
  return acc;
}

// the step index and the four head scalars a head workgroup works with
struct HeadIn {
  int step;
  float w, b, gamma, beta;
};

// the per-rating values of the scalar kinds (0 for a kind the mask does not ask for), Keras 2.12 definitions with one
// rounding per operation
template <int kAct>
__device__ __forceinline__ void metric_terms(uint32_t mask, float y, float t, float p, float (&v)[kMetricKinds]) {
#pragma clang fp contract(off)
  const float ae = fabsf(p - t);
  v[0] = ae;                                                                          // mean_absolute_error
  v[1] = (mask & ANIREC_METRIC_MAPE) ? 100.f * (ae / fmaxf(fabsf(t), kBceEps)) : 0.f;  // ..._percentage_error
  if (mask & ANIREC_METRIC_MSLE) {                                                    // ..._squared_logarithmic_error
    const float d = logf(fmaxf(p, kBceEps) + 1.f) - logf(fmaxf(t, kBceEps) + 1.f);
    v[2] = d * d;
  } else {
    v[2] = 0.f;
  }
  float l = 0.f, g;
  if (mask & ANIREC_METRIC_LOGCOSH) loss_terms<ANIREC_LOSS_LOGCOSH>(p, t, l, g);
  v[3] = l;
  v[4] = (mask & ANIREC_METRIC_BCE) ? head_loss<kAct, ANIREC_LOSS_BCE>(y, t, p) : 0.f;  // (from logits: sigmoid)
  v[5] = t == (p > 0.5f ? 1.f : 0.f) ? 1.f : 0.f;                                       // binary_accuracy
}

// AUC bucket of a prediction (Keras' evenly-spaced-thresholds path: ceil(p * (200 - 1)) - 1 in fp32, relu) and the
// fixed-point label mass of a rating; the clamps only keep a NaN or out-of-range value inside the bins
__device__ __forceinline__ int auc_bucket(float p) {
  return (int)fminf(fmaxf(ceilf(p * (float)(kAucBins - 1)) - 1.f, 0.f), (float)(kAucBins - 1));
}
__device__ __forceinline__ uint32_t auc_pos_mass(float t) {
  return (uint32_t)rintf(fminf(fmaxf(t, 0.f), 1.f) * (float)ANIREC_AUC_ONE);
}

// a workgroup's block-summed kinds into the fp64 accumulators: one atomic per requested kind (the order dependence
// stays far below the History's fp32, as in k_eval)
__device__ __forceinline__ void metric_flush(const MetricArgs &m, const float (&v)[kMetricKinds]) {
#pragma unroll
  for (int k = 0; k < kMetricKinds; ++k)
    if (m.mask & (1u << k)) atomicAdd(&m.acc->sum[k], (double)v[k]);
}

// workgroup vblk of nvb: the batch statistics (recomputed per workgroup) + 256 ratings; kAct / kLoss: the output head
// (ANIREC_ACT_* / ANIREC_LOSS_*, head_terms), one instantiation per pair.  kMetrics: also the Keras metrics of m over
// the workgroup's ratings — scratch then holds kHeadCols * 16 floats and, behind them, the zeroed 2 * kAucBins-word AUC
// histogram (k_head_metrics)
template <int kAct, int kLoss, bool kMetrics = false>
__device__ __forceinline__ void head_block(const HeadArgs &a, const HeadIn in, int vblk, int nvb, float *scratch,
                                           MetricArgs m = {}) {
  const int tid = threadIdx.x;
  const int pcap = packet_cap(a.cap);
  const int bps = (a.cap + kHeadThreads - 1) / kHeadThreads;  // blocks per segment
  const int seg = vblk / bps;
  const int i = (vblk % bps) * kHeadThreads + tid;

  // ---- issue every independent load first --------------------------------------------
  SegVals x0;
  seg_load(a.packets, pcap, x0);  // segment 0 stays in registers for both passes
  const float *mypk = a.packets + a.packet_floats * seg;
  const float my_c = i < a.cap ? mypk[i] : 0.f;
  const float my_t = i < a.cap ? mypk[pcap + i] : 0.f;
  const int step = in.step;
  const float w = in.w, b = in.b, gamma = in.gamma, beta = in.beta;
  int cnts[ANIREC_MAX_SEG];
  int n_total = 0;
#pragma unroll
  for (int s = 0; s < ANIREC_MAX_SEG; ++s) {
    cnts[s] = s < a.n_seg ? packet_count(a.packets + a.packet_floats * s, a.cap) : 0;
    n_total += cnts[s];
  }
  const float Bf = (float)n_total;

  // ---- batch statistics of z over the whole (global) batch ------------------------------------
  float mu, var;
  if (a.n_seg == 1) {
    // one rank: two passes over the 40 KB of c (registers), redundantly per workgroup
    float r[1];
    r[0] = seg_stat<false>(x0, cnts[0], w, b, 0.f);
    block_sum<1>(r, scratch);
    mu = r[0] / Bf;
    r[0] = seg_stat<true>(x0, cnts[0], w, b, mu);
    block_sum<1>(r, scratch);
    var = r[0] / Bf;  // biased (tf.nn.moments)
  } else {
    // several ranks: every packet carries (count, mean, M2) of its own z values (k_seg_stats on
    // the owning rank, same w and b everywhere); merge them in rank order (Chan et al.)
    double nsum = 0.0, msum = 0.0;
#pragma unroll
    for (int s = 0; s < ANIREC_MAX_SEG; ++s) {
      if (s < a.n_seg && cnts[s] > 0) {
        const float *tail = a.packets + a.packet_floats * s + 2 * (size_t)pcap;
        nsum += (double)cnts[s];
        msum += (double)cnts[s] * (double)tail[1];
      }
    }
    const double mean = msum / nsum;
    double m2 = 0.0;
#pragma unroll
    for (int s = 0; s < ANIREC_MAX_SEG; ++s) {
      if (s < a.n_seg && cnts[s] > 0) {
        const float *tail = a.packets + a.packet_floats * s + 2 * (size_t)pcap;
        const double dm = (double)tail[1] - mean;
        m2 += (double)tail[2] + (double)cnts[s] * dm * dm;
      }
    }
    mu = (float)mean;
    var = (float)(m2 / nsum);
  }
  const float rs = 1.0f / sqrtf(var + kBnEps);
  const float inv = rs * gamma;
  const float shift = beta - mu * inv;

  // ---- this workgroup's 256 ratings ---------------------------------------------------------
  int cnt = 0;
#pragma unroll
  for (int s = 0; s < ANIREC_MAX_SEG; ++s)
    if (s == seg) cnt = cnts[s];
  float r[kHeadCols] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float mv[kMetricKinds] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  uint32_t *hist = reinterpret_cast<uint32_t *>(scratch + kHeadCols * 16);
  if constexpr (kMetrics) __syncthreads();  // the zeroed histogram (the several-rank branch has no barrier)
  if (i < cnt) {
    const float c = my_c, t = my_t;
    const float z = c * w + b;
    const float y = z * inv + shift;
    float p, g;
    head_grad<kAct, kLoss>(y, t, p, g);
    const float dy = g / Bf;
    const float zh = (z - mu) * rs;
    r[0] = dy;
    r[1] = dy * zh;
    r[2] = head_loss<kAct, kLoss>(y, t, p);
    r[3] = (p - t) * (p - t);
    r[4] = dy * c;
    r[5] = c;
    r[6] = zh * c;
    r[7] = zh;
    if (seg == a.my_seg) a.dy[i] = dy;
    if constexpr (kMetrics) {
      metric_terms<kAct>(m.mask, y, t, p, mv);
      if (m.mask & ANIREC_METRIC_AUC) {  // LDS integer adds: order-independent
        const int bk = auc_bucket(p);
        const uint32_t wt = auc_pos_mass(t);
        atomicAdd(&hist[bk], wt);
        atomicAdd(&hist[kAucBins + bk], ANIREC_AUC_ONE - wt);
      }
    }
  }
  block_sum<kHeadCols>(r, scratch);
  const int par = step & 1;
  if (tid < kHeadCols) a.hpart[par * a.hpart_stride + (size_t)vblk * kHeadCols + tid] = r[tid];
  if constexpr (kMetrics) {
    block_sum<kMetricKinds>(mv, scratch);  // (its barriers also complete the histogram)
    if (tid == 0) metric_flush(m, mv);
    if (m.mask & ANIREC_METRIC_AUC) {
      for (int k = tid; k < 2 * kAucBins; k += kHeadThreads) {
        const uint32_t h = hist[k];
        if (h) atomicAdd(k < kAucBins ? &m.acc->auc_pos[k] : &m.acc->auc_neg[k - kAucBins], (unsigned long long)h);
      }
    }
  }

  if (vblk == 0) {
    if (tid == 0) {
      StepPub p;
      p.slot = step % a.arena_steps;
      p.n_total = n_total;
      p.n_head_blocks = nvb;
      p.step = step;
      p.alpha = a.sched[step].alpha;
      p.mu = mu;
      p.var = var;
      p.rs = rs;
      p.w = w;
      p.b = b;
      p.gamma = gamma;
      p.beta = beta;
      p.l2 = a.l2;
      p.pad0 = p.pad1 = p.pad2 = 0.f;
      a.pub[par] = p;
      a.sel[0] = step;
    }
  }
}

// (k_head and k_head_metrics are units of their own, anirec_train_head.hip and anirec_train_head_metrics.hip: their
// launches also carry the lazy update's catch-up workgroups)

}  // namespace anirec
