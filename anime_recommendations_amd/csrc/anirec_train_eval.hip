// Validation of libanirec's training path for gfx950 (MI355X): the model on held-out ratings with BatchNorm in
// inference mode, k_eval / k_eval_metrics (one instantiation per (activation, loss) pair at 128) and k_eval_w (the other
// widths, the head as run-time values), with their entry points.
#include <hip/hip_runtime.h>

#include "anirec_train_head.hpp"

namespace anirec {

// ------------------------------------------------------------------------------------
// validation (BN inference mode) and misc
// ------------------------------------------------------------------------------------
struct EvalArgs {
  const float *W;
  int n_user_rows;
  const int32_t *user_idx, *anime_idx;
  const float *rating;
  int n;
  anirec_state *state;
  int act, loss;  // ANIREC_ACT_* / ANIREC_LOSS_* of the descriptor: read by k_eval_w only
};

// the head of one validation rating: prediction, data loss and (kMetrics) the Keras metric values
template <int kAct, int kLoss, bool kMetrics>
__device__ __forceinline__ void eval_terms(uint32_t mask, float y, float t, float &p, float &li,
                                           float (&mv)[kMetricKinds]) {
  float g;
  head_grad<kAct, kLoss>(y, t, p, g);
  li = head_loss<kAct, kLoss>(y, t, p);
  if constexpr (kMetrics) metric_terms<kAct>(mask, y, t, p, mv);
}
// the same with the head as run-time values (the kernels of the other widths: one instantiation per width instead of
// one per width, activation and loss); every case is the instantiation above
template <int kAct, bool kMetrics>
__device__ __forceinline__ void eval_terms_loss(int loss, uint32_t mask, float y, float t, float &p, float &li,
                                                float (&mv)[kMetricKinds]) {
  switch (loss) {
    case ANIREC_LOSS_MSE: return eval_terms<kAct, ANIREC_LOSS_MSE, kMetrics>(mask, y, t, p, li, mv);
    case ANIREC_LOSS_MAE: return eval_terms<kAct, ANIREC_LOSS_MAE, kMetrics>(mask, y, t, p, li, mv);
    case ANIREC_LOSS_HUBER: return eval_terms<kAct, ANIREC_LOSS_HUBER, kMetrics>(mask, y, t, p, li, mv);
    case ANIREC_LOSS_LOGCOSH: return eval_terms<kAct, ANIREC_LOSS_LOGCOSH, kMetrics>(mask, y, t, p, li, mv);
    default: return eval_terms<kAct, ANIREC_LOSS_BCE, kMetrics>(mask, y, t, p, li, mv);
  }
}
template <bool kMetrics>
__device__ __forceinline__ void eval_terms_any(int act, int loss, uint32_t mask, float y, float t, float &p, float &li,
                                               float (&mv)[kMetricKinds]) {
  switch (act) {
    case ANIREC_ACT_LINEAR: return eval_terms_loss<ANIREC_ACT_LINEAR, kMetrics>(loss, mask, y, t, p, li, mv);
    case ANIREC_ACT_TANH: return eval_terms_loss<ANIREC_ACT_TANH, kMetrics>(loss, mask, y, t, p, li, mv);
    case ANIREC_ACT_RELU: return eval_terms_loss<ANIREC_ACT_RELU, kMetrics>(loss, mask, y, t, p, li, mv);
    case ANIREC_ACT_SOFTPLUS: return eval_terms_loss<ANIREC_ACT_SOFTPLUS, kMetrics>(loss, mask, y, t, p, li, mv);
    default: return eval_terms_loss<ANIREC_ACT_SIGMOID, kMetrics>(loss, mask, y, t, p, li, mv);
  }
}

// one row group per validation rating (1024 / kD ratings per workgroup).  kAct / kLoss >= 0: the head as template
// parameters (k_eval, k_eval_metrics: the 128-wide kernels); < 0: a.act / a.loss (k_eval_w).  kMetrics: also the Keras
// metrics of m
template <int kAct, int kLoss, bool kMetrics, int kD>
__device__ __forceinline__ void eval_body(const EvalArgs &a, const MetricArgs &m) {
  constexpr int kG = kD / 4, kRpb = 256 / kG;
  __shared__ float sh[kMetrics ? 2 + kMetricKinds : 2][kRpb];
  const anirec_state *st = a.state;
  const float w = st->w, b = st->b;
  const float inv = st->gamma * (1.0f / sqrtf(st->mov_var + kBnEps));
  const float shift = st->beta - st->mov_mean * inv;
  const int l32 = threadIdx.x & (kG - 1), h = threadIdx.x / kG;
  const int i = blockIdx.x * kRpb + h;
  float li = 0.f, se = 0.f;
  float mv[kMetricKinds] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (i < a.n) {
    float su, sa, dd;
    pair_dots<kD>(reinterpret_cast<const float4 *>(a.W), a.user_idx[i], a.anime_idx[i] + a.n_user_rows,
                  l32, su, sa, dd);
    const float c = cos_from_dots(su, sa, dd);
    const float y = (c * w + b) * inv + shift;
    const float t = a.rating[i];
    float p;
    if constexpr (kAct >= 0) eval_terms<kAct, kLoss, kMetrics>(m.mask, y, t, p, li, mv);
    else eval_terms_any<kMetrics>(a.act, a.loss, m.mask, y, t, p, li, mv);
    se = (p - t) * (p - t);
    if constexpr (kMetrics) {
      if ((m.mask & ANIREC_METRIC_AUC) && l32 == 0) {  // a few ratings a workgroup: straight into the integer bins
        const int bk = auc_bucket(p);
        const uint32_t wt = auc_pos_mass(t);
        if (wt) atomicAdd(&m.acc->auc_pos[bk], (unsigned long long)wt);
        if (wt != ANIREC_AUC_ONE) atomicAdd(&m.acc->auc_neg[bk], (unsigned long long)(ANIREC_AUC_ONE - wt));
      }
    }
  }
  if (l32 == 0) {
    sh[0][h] = li;
    sh[1][h] = se;
    if constexpr (kMetrics) {
#pragma unroll
      for (int k = 0; k < kMetricKinds; ++k) sh[2 + k][h] = mv[k];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double L = 0., E = 0.;
    for (int k = 0; k < kRpb; ++k) {
      L += sh[0][k];
      E += sh[1][k];
    }
    // fp64 atomics: order-dependent only below 1e-16 relative, far under the fp32 History values
    atomicAdd(&a.state->val_bce_sum, L);
    atomicAdd(&a.state->val_se_sum, E);
    if (blockIdx.x == 0) atomicAdd(&a.state->val_n, (double)a.n);
    if constexpr (kMetrics) {
#pragma unroll
      for (int k = 0; k < kMetricKinds; ++k) {
        if (!(m.mask & (1u << k))) continue;
        double v = 0.;
        for (int j = 0; j < kRpb; ++j) v += sh[2 + k][j];
        atomicAdd(&m.acc->sum[k], v);
      }
    }
  }
}

template <int kAct, int kLoss>
__global__ __launch_bounds__(256) void k_eval(EvalArgs a) {
  eval_body<kAct, kLoss, false, kDim>(a, MetricArgs{});
}

// k_eval that also adds the Keras metrics of m (anirec_eval_metrics)
template <int kAct, int kLoss>
__global__ __launch_bounds__(256) void k_eval_metrics(EvalArgs a, MetricArgs m) {
  eval_body<kAct, kLoss, true, kDim>(a, m);
}

// validation at another width (anirec_eval_metrics_w), the head from a.act / a.loss
template <bool kMetrics, int kD>
__global__ __launch_bounds__(256) void k_eval_w(EvalArgs a, MetricArgs m) {
  eval_body<-1, -1, kMetrics, kD>(a, m);
}

}  // namespace anirec

using namespace anirec;

extern "C" {

int anirec_eval(const anirec_train_desc *d, const int32_t *user_idx, const int32_t *anime_idx,
                const float *rating, int32_t n, void *stream) {
  return anirec_eval_metrics(d, 0, nullptr, user_idx, anime_idx, rating, n, stream);
}

int anirec_eval_metrics(const anirec_train_desc *d, uint32_t mask, anirec_metric_acc *acc, const int32_t *user_idx,
                        const int32_t *anime_idx, const float *rating, int32_t n, void *stream) {
  return anirec_eval_metrics_w(d, ANIREC_DIM, mask, acc, user_idx, anime_idx, rating, n, stream);
}

int anirec_eval_metrics_w(const anirec_train_desc *d, int32_t dim, uint32_t mask, anirec_metric_acc *acc,
                          const int32_t *user_idx, const int32_t *anime_idx, const float *rating, int32_t n,
                          void *stream) {
  if (!dim_ok(dim) || !d || !d->W || !d->state || !user_idx || !anime_idx || !rating || n < 0 || check_opt(d))
    return ANIREC_EINVAL;
  if (check_metrics(d, mask)) return ANIREC_EINVAL;
  const MetricArgs m = (mask && acc) ? MetricArgs{mask, acc} : MetricArgs{};
  if (n == 0) return ANIREC_OK;
  EvalArgs a;
  a.W = d->W;
  a.n_user_rows = d->n_user_rows;
  a.user_idx = user_idx;
  a.anime_idx = anime_idx;
  a.rating = rating;
  a.n = n;
  a.state = d->state;
  a.act = d->activation;
  a.loss = d->loss;
  if (dim != kDim) {  // the head as run-time values: one kernel per width
    with_width(dim, [&](auto kd) {
      constexpr int kD = decltype(kd)::value, kRpb = 1024 / kD;
      if constexpr (kD != kDim) {  // (nothing of k_eval_w is instantiated at 128)
        const dim3 grid((n + kRpb - 1) / kRpb);
        if (m.mask) hipLaunchKernelGGL((k_eval_w<true, kD>), grid, dim3(256), 0, (hipStream_t)stream, a, m);
        else hipLaunchKernelGGL((k_eval_w<false, kD>), grid, dim3(256), 0, (hipStream_t)stream, a, m);
      }
    });
    return (int)hipGetLastError();
  }
  with_act(d->activation, [&](auto act) {
    with_loss(d->loss, [&](auto loss) {
      if (m.mask)
        hipLaunchKernelGGL((k_eval_metrics<decltype(act)::value, decltype(loss)::value>), dim3((n + 7) / 8),
                           dim3(256), 0, (hipStream_t)stream, a, m);
      else
        hipLaunchKernelGGL((k_eval<decltype(act)::value, decltype(loss)::value>), dim3((n + 7) / 8), dim3(256), 0,
                           (hipStream_t)stream, a);
    });
  });
  return (int)hipGetLastError();
}

}  // extern "C"
