// Fold-in of new users for gfx950 (MI355X): fit one fresh user-embedding row per new user to that user's own ratings,
// every other layer of the model frozen (include/anirec.h, anirec_fold_in).
//
// The Keras model of neural_network.py:66-106 with the anime table, Dense(1) and BatchNorm (inference mode) frozen;
// model.fit full-batch on the user's n ratings with Keras-2.12 Adam, `steps` iterations.  The fits of different users
// share nothing but the frozen table, so a call is
//   pre-pass   Ah = l2-normalised anime rows into the workspace, once (rownorm_body<1>, the train step's forward form)
//   k_fold_in  one workgroup of 256 lanes per user, every step inside the one launch.  A row is one float4 per lane of a
//              group of kG = width / 4 lanes; the workgroup holds kNG = 256 / kG groups (32, 16, 8, 4 at widths 32, 64,
//              128, 256).  EVERY group keeps the user's u, m, v in registers (identical copies).  Per step, group g walks
//              ratings g, g + kNG, ... of the list in that order: gathers Ah[a_i], the cosine by the group butterfly, the
//              head, and adds dc_i (ah_i - c_i uh) to its float4 accumulator.  The kNG partial rows and loss sums meet in
//              LDS: every lane adds the kNG values of its column in group order 0 .. kNG-1, so all groups hold the same
//              gradient and take the same Adam step.  No atomics; the order depends on nothing but the user's own list:
//              a user's result is the same bits run to run, alone or in any batch, at any position.
// LDS: 256 float4 + kNG floats (4.1 KB at most) per workgroup; the Ah rows are not staged (they come through L2: a
// 17 560 x 128 table is 9 MB), so a list of any length takes the one path.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "anirec_dev.hpp"

namespace anirec {

struct FoldArgs {
  const float *Ah;          // [n_anime][dim] normalised anime rows (workspace)
  int n_anime;
  const int64_t *offsets;   // [n_new + 1]
  const int32_t *anime_idx;
  const float *rating;
  const float *init;        // [n_new][dim]
  const float *alpha;       // [steps]
  int steps;
  float hs, hb, l2;
  int act, loss;
  float *out_rows;          // [n_new][dim]
  float *out_loss;          // [n_new]
  int32_t *err;
};

// one rating through the head chosen at run time: p, dl/dy and the data loss by head_grad / head_loss of that pair
// (the switch is uniform over the launch)
__device__ __forceinline__ void head_any(int act, int loss, float y, float t, float &g, float &l) {
  float p;
#define ANIREC_FOLD_CASE(A, L)                    \
  case (A)*8 + (L):                               \
    head_grad<(A), (L)>(y, t, p, g);              \
    l = head_loss<(A), (L)>(y, t, p);             \
    break;
#define ANIREC_FOLD_ACT(A)                                                                   \
  ANIREC_FOLD_CASE(A, ANIREC_LOSS_BCE) ANIREC_FOLD_CASE(A, ANIREC_LOSS_MSE)                  \
  ANIREC_FOLD_CASE(A, ANIREC_LOSS_MAE) ANIREC_FOLD_CASE(A, ANIREC_LOSS_HUBER)                \
  ANIREC_FOLD_CASE(A, ANIREC_LOSS_LOGCOSH)
  switch (act * 8 + loss) {
    ANIREC_FOLD_ACT(ANIREC_ACT_LINEAR)
    ANIREC_FOLD_ACT(ANIREC_ACT_TANH)
    ANIREC_FOLD_ACT(ANIREC_ACT_RELU)
    ANIREC_FOLD_ACT(ANIREC_ACT_SOFTPLUS)
    ANIREC_FOLD_CASE(ANIREC_ACT_SIGMOID, ANIREC_LOSS_MSE)
    ANIREC_FOLD_CASE(ANIREC_ACT_SIGMOID, ANIREC_LOSS_MAE)
    ANIREC_FOLD_CASE(ANIREC_ACT_SIGMOID, ANIREC_LOSS_HUBER)
    ANIREC_FOLD_CASE(ANIREC_ACT_SIGMOID, ANIREC_LOSS_LOGCOSH)
    default:
      head_grad<ANIREC_ACT_SIGMOID, ANIREC_LOSS_BCE>(y, t, p, g);
      l = head_loss<ANIREC_ACT_SIGMOID, ANIREC_LOSS_BCE>(y, t, p);
      break;
  }
#undef ANIREC_FOLD_ACT
#undef ANIREC_FOLD_CASE
}

template <int kD>
__global__ __launch_bounds__(256) void k_fold_in(FoldArgs a) {
#pragma clang fp contract(off)
  constexpr int kG = kD / 4, kNG = 256 / kG;
  __shared__ __attribute__((aligned(16))) float4 red[256];  // [kNG][kG]: the groups' partial gradient rows
  __shared__ float lred[kNG];                               // the groups' partial loss sums
  const int tid = threadIdx.x, l = tid & (kG - 1), g = tid / kG;
  const size_t u = blockIdx.x;
  float4 *out4 = reinterpret_cast<float4 *>(a.out_rows) + u * kG;
  const float4 w0 = reinterpret_cast<const float4 *>(a.init)[u * kG + l];
  const float qnan = __uint_as_float(0x7FC00000u);
  const long long lo = a.offsets[u], hi = a.offsets[u + 1];
  const bool bad_range = lo < 0 || hi < lo || hi - lo > (long long)INT_MAX;
  if (!bad_range && hi == lo) {  // no ratings: the start row bit for bit, no loss to report
    if (g == 0) out4[l] = w0;
    if (tid == 0) a.out_loss[u] = qnan;
    return;
  }
  // nothing is read through a bad offset pair or a bad index: the whole list is checked before any row is gathered
  const int n = bad_range ? 0 : (int)(hi - lo);
  const int32_t *ai = a.anime_idx + (bad_range ? 0 : lo);
  const float *rt = a.rating + (bad_range ? 0 : lo);
  int bad = bad_range ? 1 : 0;
  for (int i = tid; i < n; i += 256) bad |= ((uint32_t)ai[i] >= (uint32_t)a.n_anime) ? 1 : 0;
  if (__syncthreads_or(bad)) {
    if (g == 0) out4[l] = make_float4(qnan, qnan, qnan, qnan);
    if (tid == 0) {
      a.out_loss[u] = qnan;
      *a.err = 1;
    }
    return;
  }
  const float4 *Ah4 = reinterpret_cast<const float4 *>(a.Ah);
  const float nf = (float)n, two_l2 = 2.0f * a.l2;
  float4 w = w0;
  float4 m = make_float4(0.f, 0.f, 0.f, 0.f), v = m;
  for (int s = 0;; ++s) {
    const float ss = group_sum<kG>(w.x * w.x + w.y * w.y + w.z * w.z + w.w * w.w);
    const float ru = 1.0f / sqrtf(fmaxf(ss, kL2nEps));
    const float4 uh = make_float4(w.x * ru, w.y * ru, w.z * ru, w.w * ru);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float lsum = 0.f;
    for (int i = g; i < n; i += kNG) {
      const float4 x = Ah4[(size_t)ai[i] * kG + l];
      const float t = rt[i];
      const float c = group_sum<kG>(uh.x * x.x + uh.y * x.y + uh.z * x.z + uh.w * x.w);
      const float y = __fmaf_rn(c, a.hs, a.hb);
      float gy, li;
      head_any(a.act, a.loss, y, t, gy, li);
      lsum += li;
      const float dc = (gy / nf) * a.hs;
      acc.x += dc * (x.x - c * uh.x);
      acc.y += dc * (x.y - c * uh.y);
      acc.z += dc * (x.z - c * uh.z);
      acc.w += dc * (x.w - c * uh.w);
    }
    red[tid] = acc;
    if (l == 0) lred[g] = lsum;
    __syncthreads();
    float4 gs = red[l];
    float lt = lred[0];
#pragma unroll 4
    for (int k = 1; k < kNG; ++k) {  // fixed order: group 0, 1, ..., the same in every group
      const float4 q = red[k * kG + l];
      gs.x += q.x;
      gs.y += q.y;
      gs.z += q.z;
      gs.w += q.w;
      lt += lred[k];
    }
    __syncthreads();  // red / lred are rewritten by the next step
    if (s >= a.steps) {  // the loss at the row the last step left
      if (g == 0) out4[l] = w;
      if (tid == 0) a.out_loss[u] = lt / nf + a.l2 * ss;
      return;
    }
    const float al = a.alpha[s];
    adam_elem(w.x, m.x, v.x, ru * gs.x + two_l2 * w.x, al);
    adam_elem(w.y, m.y, v.y, ru * gs.y + two_l2 * w.y, al);
    adam_elem(w.z, m.z, v.z, ru * gs.z + two_l2 * w.z, al);
    adam_elem(w.w, m.w, v.w, ru * gs.w + two_l2 * w.w, al);
  }
}

static size_t fold_bytes(int32_t n_anime, int32_t dim) { return (size_t)n_anime * (size_t)dim * sizeof(float); }

}  // namespace anirec

using namespace anirec;

extern "C" {

size_t anirec_fold_in_workspace_bytes(int32_t n_anime, int32_t n_new, int32_t dim) {
  if (n_anime < 1 || n_new < 0 || !dim_ok(dim)) return 0;
  return fold_bytes(n_anime, dim);
}

int anirec_fold_in(const float *A, int32_t dim, int32_t n_anime, const anirec_head *head, int32_t activation,
                   int32_t loss, float l2, const int64_t *offsets, const int32_t *anime_idx, const float *rating,
                   int32_t n_new, const float *init, const float *alpha, int32_t steps, float *out_rows,
                   float *out_loss, int32_t *err_flag, void *workspace, size_t workspace_bytes, void *stream) {
  if (!dim_ok(dim) || !act_ok(activation) || !loss_ok(loss) || n_anime < 1 || n_new < 0 || steps < 0)
    return ANIREC_EINVAL;
  if (n_new == 0) return ANIREC_OK;
  if (!A || !head || !offsets || !init || !out_rows || !out_loss || !err_flag || !workspace || (steps > 0 && !alpha))
    return ANIREC_EINVAL;
  if (workspace_bytes < fold_bytes(n_anime, dim)) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  float *Ah = (float *)workspace;
  l2norm_rows(A, n_anime, Ah, dim, s);
  ANIREC_HIP_CHECK(hipGetLastError());
  FoldArgs a;
  a.Ah = Ah;
  a.n_anime = n_anime;
  a.offsets = offsets;
  a.anime_idx = anime_idx;
  a.rating = rating;
  a.init = init;
  a.alpha = alpha;
  a.steps = steps;
  head_affine_f32(head, &a.hs, &a.hb);
  a.l2 = l2;
  a.act = activation;
  a.loss = loss;
  a.out_rows = out_rows;
  a.out_loss = out_loss;
  a.err = err_flag;
  auto launch = [&](auto kd) {
    hipLaunchKernelGGL(k_fold_in<decltype(kd)::value>, dim3((unsigned)n_new), dim3(256), 0, s, a);
  };
  if (dim == kDim)
    launch(std::integral_constant<int, kDim>());
  else
    with_width(dim, launch);
  return (int)hipGetLastError();
}

}  // extern "C"
