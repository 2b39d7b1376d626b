// Device-side helpers shared by the gfx950 kernels of libanirec.
// Wave = 64 lanes on CDNA4; a 128-float embedding row is one float4 per lane of a
// HALF-wave (32 lanes x 16 B = 512 B, one fully coalesced request).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/anirec.h"

#define ANIREC_HIP_CHECK(expr)                  \
  do {                                          \
    hipError_t _e = (expr);                     \
    if (_e != hipSuccess) return (int)_e;       \
  } while (0)

namespace anirec {

constexpr int kDim = ANIREC_DIM;
constexpr int kRowVec = kDim / 4;  // float4 per row = 32 = half-wave
constexpr float kL2nEps = 1e-12f;  // tf.nn.l2_normalize epsilon (Dot(normalize=True))
constexpr float kBnEps = 1e-3f;    // BatchNormalization epsilon
constexpr float kBnDecay = 0.01f;  // 1 - momentum(0.99)
constexpr float kOneMinusB1 = 0.1f;    // float32(1 - 0.9)
constexpr float kOneMinusB2 = 0.001f;  // float32(1 - 0.999)
constexpr float kAdamEps = 1e-7f;

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// Sum over the 32 lanes of a half-wave (lanes [0,32) and [32,64) reduce separately);
// every lane of the half receives the total.  Fixed butterfly order -> deterministic.
__device__ __forceinline__ float halfwave_sum(float v) {
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 32);
  return v;
}

// Sum over the kG lanes of a row group (kG = width / 4 = 8, 16, 32 or 64 lanes: 8, 4, 2 or 1 rows per wave); every
// lane of the group receives the total.  kG == 32 is halfwave_sum, butterfly step for step; kG == 64 crosses the two
// 32-lane halves of the wave.
template <int kG>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = kG / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, kG);
  return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Block-wide sum of N floats per thread (blockDim.x multiple of 64, <= 1024).
// `scratch` needs N*16 floats.  Result broadcast to every thread.
template <int N>
__device__ __forceinline__ void block_sum(float (&v)[N], float *scratch) {
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = wave_sum(v[i]);
  __syncthreads();  // scratch may still be read from a previous call
  if (lane_id() == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) scratch[i * 16 + w] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float s = 0.f;
    for (int k = 0; k < nw; ++k) s += scratch[i * 16 + k];  // fixed order
    v[i] = s;
  }
}

// IEEE, never contracted into FMA (HIP's __fmul_rn/__fadd_rn are plain operators and hipcc
// defaults to -ffp-contract=fast, so contraction is switched off per block): the fused Adam
// must be bit-identical to the NumPy fp32 oracle given the same gradient.
__device__ __forceinline__ void adam_elem(float &w, float &m, float &v, float g, float alpha) {
#pragma clang fp contract(off)
  m = m + (g - m) * kOneMinusB1;
  v = v + (g * g - v) * kOneMinusB2;
  w = w - (m * alpha) / (sqrtf(v) + kAdamEps);
}

// The one-slot Keras-2.12 optimisers (include/anirec.h, ANIREC_OPT_*), the same rules: `s` is the RMSprop velocity /
// the Adagrad accumulator, `lr` the schedule's rate.  Keras takes tf.math.rsqrt; here it is the correctly rounded
// 1/sqrtf, so that a NumPy restatement holds the kernels bitwise.
constexpr float kRmsRho = 0.9f;
constexpr float kRmsOneMinusRho = 0.1f;  // float32(1 - 0.9)
__device__ __forceinline__ void sgd_elem(float &w, float g, float lr) {
#pragma clang fp contract(off)
  w = w - g * lr;
}
__device__ __forceinline__ void rmsprop_elem(float &w, float &s, float g, float lr) {
#pragma clang fp contract(off)
  s = kRmsRho * s + kRmsOneMinusRho * (g * g);
  w = w - (lr * g) * (1.0f / sqrtf(s + kAdamEps));
}
__device__ __forceinline__ void adagrad_elem(float &w, float &s, float g, float lr) {
#pragma clang fp contract(off)
  s = s + g * g;
  w = w - (lr * g) / sqrtf(s + kAdamEps);
}
// one element of any kind, chosen at compile time: m is Adam's first moment, v its second / the one slot
template <int kOpt>
__device__ __forceinline__ void opt_elem(float &w, float &m, float &v, float g, float rate) {
  if constexpr (kOpt == ANIREC_OPT_ADAM) {
    adam_elem(w, m, v, g, rate);
  } else if constexpr (kOpt == ANIREC_OPT_SGD) {
    sgd_elem(w, g, rate);
  } else if constexpr (kOpt == ANIREC_OPT_RMSPROP) {
    rmsprop_elem(w, v, g, rate);
  } else {
    static_assert(kOpt == ANIREC_OPT_ADAGRAD, "unknown optimiser kind");
    adagrad_elem(w, v, g, rate);
  }
}

// g_total = (g_sparse - s*w) + two_l2*w with every product and sum rounded once.
__device__ __forceinline__ float grad_total(float gs, float s, float w, float two_l2) {
#pragma clang fp contract(off)
  return (gs - s * w) + two_l2 * w;
}

__device__ __forceinline__ float sigmoidf_stable(float y) {
  float e = __expf(-fabsf(y));
  // expf via the fast path is within 2 ulp; the 1e-5 tolerance on ratings absorbs it
  return y >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

// tf.nn.sigmoid_cross_entropy_with_logits: the binary_crossentropy of the sigmoid head (Keras takes the logits)
__device__ __forceinline__ float bce_logits(float y, float t) {
  return fmaxf(y, 0.f) - y * t + log1pf(expf(-fabsf(y)));
}

// ---- the output head (include/anirec.h, ANIREC_ACT_* / ANIREC_LOSS_*): ONE definition per kind, shared by the
// training head, validation and every predict path.  Outside the default sigmoid + BCE pair (whose code the kernels keep
// as it was: from logits, dy = (p - t) / B) every product and sum is rounded once, so that a NumPy restatement in the
// same order holds them to a few ulps of the transcendental functions.
constexpr float kBceEps = 1e-7f;                // Keras backend.epsilon()
constexpr float kBceOneMinusEps = 1.0f - 1e-7f; // rounded in fp32, as tf.clip_by_value's 1 - epsilon
constexpr float kLn2 = 0.693147180559945309f;

__device__ __forceinline__ float softplusf_stable(float x) {
#pragma clang fp contract(off)
  return fmaxf(x, 0.f) + log1pf(__expf(-fabsf(x)));
}

// p = act(y): every kind is non-decreasing in y (the top-k paths rely on it)
template <int kAct>
__device__ __forceinline__ float act_fwd(float y) {
  if constexpr (kAct == ANIREC_ACT_SIGMOID) {
    return sigmoidf_stable(y);
  } else if constexpr (kAct == ANIREC_ACT_LINEAR) {
    return y;
  } else if constexpr (kAct == ANIREC_ACT_TANH) {
    return tanhf(y);
  } else if constexpr (kAct == ANIREC_ACT_RELU) {
    return fmaxf(y, 0.f);
  } else {
    static_assert(kAct == ANIREC_ACT_SOFTPLUS, "unknown activation");
    return softplusf_stable(y);
  }
}

// p = act(y) with the activation either a compile-time constant (kAct >= 0: the 128-wide kernels, one instantiation
// per kind as ever) or, kAct < 0, the run-time value `act` (the kernels of the other widths: one instantiation per
// width, not per width and kind).  The same act_fwd either way.
template <int kAct>
__device__ __forceinline__ float act_any(float y, int act) {
  if constexpr (kAct >= 0) {
    return act_fwd<kAct>(y);
  } else {
    switch (act) {
      case ANIREC_ACT_LINEAR: return act_fwd<ANIREC_ACT_LINEAR>(y);
      case ANIREC_ACT_TANH: return act_fwd<ANIREC_ACT_TANH>(y);
      case ANIREC_ACT_RELU: return act_fwd<ANIREC_ACT_RELU>(y);
      case ANIREC_ACT_SOFTPLUS: return act_fwd<ANIREC_ACT_SOFTPLUS>(y);
      default: return act_fwd<ANIREC_ACT_SIGMOID>(y);
    }
  }
}

// d act / d y as TF's gradient op computes it, from y and p = act(y)
template <int kAct>
__device__ __forceinline__ float act_grad(float y, float p) {
#pragma clang fp contract(off)
  if constexpr (kAct == ANIREC_ACT_SIGMOID) {
    return p * (1.f - p);
  } else if constexpr (kAct == ANIREC_ACT_LINEAR) {
    return 1.f;
  } else if constexpr (kAct == ANIREC_ACT_TANH) {
    return 1.f - p * p;
  } else if constexpr (kAct == ANIREC_ACT_RELU) {
    return y > 0.f ? 1.f : 0.f;
  } else {
    static_assert(kAct == ANIREC_ACT_SOFTPLUS, "unknown activation");
    return sigmoidf_stable(y);
  }
}

// the loss l(p, t) of one rating and dl/dp (the probability form of BCE: outside the sigmoid head)
template <int kLoss>
__device__ __forceinline__ void loss_terms(float p, float t, float &l, float &g) {
#pragma clang fp contract(off)
  const float e = p - t;
  if constexpr (kLoss == ANIREC_LOSS_BCE) {
    const float q = fminf(fmaxf(p, kBceEps), kBceOneMinusEps);
    const float a = q + kBceEps, b = (1.f - q) + kBceEps;
    l = -(t * logf(a) + (1.f - t) * logf(b));
    // tf.clip_by_value's gradient passes on the closed interval [eps, 1 - eps] (a NaN p passes nothing)
    g = (p >= kBceEps && p <= kBceOneMinusEps) ? -(t / a) + (1.f - t) / b : 0.f;
  } else if constexpr (kLoss == ANIREC_LOSS_MSE) {
    l = e * e;
    g = 2.f * e;
  } else if constexpr (kLoss == ANIREC_LOSS_MAE) {
    l = fabsf(e);
    g = e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
  } else if constexpr (kLoss == ANIREC_LOSS_HUBER) {
    const float ae = fabsf(e);
    l = ae <= 1.f ? 0.5f * (e * e) : ae - 0.5f;
    g = ae <= 1.f ? e : (e > 0.f ? 1.f : -1.f);
  } else {
    static_assert(kLoss == ANIREC_LOSS_LOGCOSH, "unknown loss");
    l = (e + softplusf_stable(-2.f * e)) - kLn2;
    g = 1.f - 2.f * sigmoidf_stable(-2.f * e);
  }
}

// one rating through the head: p = act(y) and dl/dy (the 1/B of the batch mean not applied) ...
template <int kAct, int kLoss>
__device__ __forceinline__ void head_grad(float y, float t, float &p, float &g) {
#pragma clang fp contract(off)
  p = act_fwd<kAct>(y);
  if constexpr (kAct == ANIREC_ACT_SIGMOID && kLoss == ANIREC_LOSS_BCE) {
    g = p - t;
  } else {
    float l, gp;
    loss_terms<kLoss>(p, t, l, gp);
    g = gp * act_grad<kAct>(y, p);
  }
}
// ... and its data loss
template <int kAct, int kLoss>
__device__ __forceinline__ float head_loss(float y, float t, float p) {
  if constexpr (kAct == ANIREC_ACT_SIGMOID && kLoss == ANIREC_LOSS_BCE) {
    return bce_logits(y, t);
  } else {
    float l, gp;
    loss_terms<kLoss>(p, t, l, gp);
    return l;
  }
}

// rating of a pair from its cosine through the folded BN-inference head: ONE definition shared by the
// exact path (k_scores epilogue) and the MFMA path's re-rank, so both produce the same fp32 value
// (kAct < 0: the run-time activation `act`, act_any)
template <int kAct = ANIREC_ACT_SIGMOID>
__device__ __forceinline__ float rating_from_cosine(float c, float hs, float hb, int act = 0) {
  return act_any<kAct>(__fmaf_rn(c, hs, hb), act);
}

// ---- the greedy re-ranks (anirec_mmr_rerank, anirec_calibrate_rerank): one order of the candidates' values, one
// rounding of a value, one wave-wide max
// larger val -> larger key; NaN -> 1 (after every number); -0 and +0 share a key; 0 is "not a candidate"
__device__ __forceinline__ uint32_t mmr_key(float v) {
  if (v != v) return 1u;
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7FFFFFFFu) == 0u) u = 0u;
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return u < 2u ? 2u : u;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// val_i = (lambda * score_i) - (oml * pen_i): each product rounded, then the difference
__device__ __forceinline__ float mmr_val(float ls, float oml, float pen) {
#pragma clang fp contract(off)
  return ls - oml * pen;
}
__device__ __forceinline__ float mmr_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// ---- the order of a score row (the exact select of anirec_infer.hip, the fusion of anirec_fuse.hip): one key, one sort
// larger score -> larger key; NaN -> 1 (ranks after every number); 0 is "not a candidate"
__device__ __forceinline__ uint32_t score_key(float s) {
  if (s != s) return 1u;
  uint32_t u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return u < 2u ? 2u : u;
}

constexpr int kLdsSortMax = 20480;  // one-workgroup sort: 20480 x 8 B = the 160 KiB of LDS one workgroup may hold

// Sort in LDS, descending, of sw[0 .. cnt) by the whole workgroup (thread tid of nt): a bitonic network in its
// one-direction form (each merge starts by comparing mirrored pairs), so the entries past the count are virtual zeros
// that no comparator moves and are skipped.  The entries must be in place behind a barrier; every pass ends with one
// (cnt < 2 has no pass).
__device__ __forceinline__ void lds_sort_desc(unsigned long long *sw, uint32_t cnt, int tid, int nt) {
  uint32_t npad = 1;
  while (npad < cnt) npad <<= 1;
  for (uint32_t lg = 1; (1u << lg) <= npad; ++lg) {
    const uint32_t size = 1u << lg, half = size >> 1;
    for (uint32_t p = tid; p < npad / 2; p += nt) {
      const uint32_t base = (p >> (lg - 1)) << lg, off = p & (half - 1);
      const uint32_t x = base + off, y = base + size - 1 - off;
      if (y < cnt) {
        const unsigned long long u = sw[x], v = sw[y];
        if (u < v) {
          sw[x] = v;
          sw[y] = u;
        }
      }
    }
    __syncthreads();
    for (uint32_t stride = size >> 2; stride > 0; stride >>= 1) {
      for (uint32_t p = tid; p < npad / 2; p += nt) {
        const uint32_t x = 2 * p - (p & (stride - 1)), y = x + stride;
        if (y < cnt) {
          const unsigned long long u = sw[x], v = sw[y];
          if (u < v) {
            sw[x] = v;
            sw[y] = u;
          }
        }
      }
      __syncthreads();
    }
  }
}

// host: a row width the *_w entry points implement (a row is dim / 4 lanes of float4: 8, 16, 32 or 64 lanes)
static inline bool dim_ok(int32_t dim) { return dim == 32 || dim == 64 || dim == 128 || dim == 256; }
// host: calls f(std::integral_constant<int, kD>) with a (checked) width as a compile-time constant.  A kernel that
// exists off 128 only (the run-time-head kernels, whose 128 form takes the head as template constants) is launched
// under `if constexpr (kD != kDim)` inside f, so nothing of it is instantiated at 128.
template <typename F>
static inline void with_width(int32_t dim, F &&f) {
  switch (dim) {
    case 32: f(std::integral_constant<int, 32>()); break;
    case 64: f(std::integral_constant<int, 64>()); break;
    case 128: f(std::integral_constant<int, 128>()); break;
    case 256: f(std::integral_constant<int, 256>()); break;
    default: break;
  }
}

// host: out[r] = W[r] * (1 / sqrt(max(sum W[r]^2, 1e-12))) for n rows of a (checked) width, enqueued on s: the
// tf.nn.l2_normalize rows of rownorm_body<1> (defined in anirec_infer.hip, beside the kernels it launches)
void l2norm_rows(const float *W, int n, float *out, int dim, hipStream_t s);

// host: an ANIREC_ACT_* / ANIREC_LOSS_* value the kernels implement
static inline bool act_ok(int32_t a) { return a >= ANIREC_ACT_SIGMOID && a <= ANIREC_ACT_SOFTPLUS; }
static inline bool loss_ok(int32_t l) { return l >= ANIREC_LOSS_BCE && l <= ANIREC_LOSS_LOGCOSH; }

// host: calls f(std::integral_constant<int, kAct>) with the activation as a compile-time constant
template <typename F>
static inline auto with_act(int32_t act, F &&f) {
  switch (act) {
    case ANIREC_ACT_LINEAR: return f(std::integral_constant<int, ANIREC_ACT_LINEAR>());
    case ANIREC_ACT_TANH: return f(std::integral_constant<int, ANIREC_ACT_TANH>());
    case ANIREC_ACT_RELU: return f(std::integral_constant<int, ANIREC_ACT_RELU>());
    case ANIREC_ACT_SOFTPLUS: return f(std::integral_constant<int, ANIREC_ACT_SOFTPLUS>());
    default: return f(std::integral_constant<int, ANIREC_ACT_SIGMOID>());
  }
}
template <typename F>
static inline auto with_loss(int32_t loss, F &&f) {
  switch (loss) {
    case ANIREC_LOSS_MSE: return f(std::integral_constant<int, ANIREC_LOSS_MSE>());
    case ANIREC_LOSS_MAE: return f(std::integral_constant<int, ANIREC_LOSS_MAE>());
    case ANIREC_LOSS_HUBER: return f(std::integral_constant<int, ANIREC_LOSS_HUBER>());
    case ANIREC_LOSS_LOGCOSH: return f(std::integral_constant<int, ANIREC_LOSS_LOGCOSH>());
    default: return f(std::integral_constant<int, ANIREC_LOSS_BCE>());
  }
}
// host: calls f(std::integral_constant<int, kOpt>) with the update rule (ANIREC_OPT_*) as a compile-time constant
template <typename F>
static inline auto with_opt(int32_t kind, F &&f) {
  switch (kind) {
    case ANIREC_OPT_SGD: return f(std::integral_constant<int, ANIREC_OPT_SGD>());
    case ANIREC_OPT_RMSPROP: return f(std::integral_constant<int, ANIREC_OPT_RMSPROP>());
    case ANIREC_OPT_ADAGRAD: return f(std::integral_constant<int, ANIREC_OPT_ADAGRAD>());
    default: return f(std::integral_constant<int, ANIREC_OPT_ADAM>());
  }
}

// sigmoid(gamma*(w*c+b-mu)/sqrt(var+eps)+beta) = sigmoid(c*hs + hb); folded in fp32 exactly as
// tf.nn.batch_normalization does: inv = rsqrt(var+eps)*gamma; y = z*inv + (beta - mu*inv)
static inline void head_affine_f32(const anirec_head *h, float *hs, float *hb) {
  const float inv = (1.0f / sqrtf(h->mov_var + kBnEps)) * h->gamma;
  *hs = h->w * inv;
  *hb = h->b * inv + (h->beta - h->mov_mean * inv);
}

}  // namespace anirec
