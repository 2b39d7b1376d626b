// Content-based score rows from TF-IDF item vectors, for gfx950 (MI355X): include/anirec.h, anirec_content_scores.
// A user profile is a weighted sum of sparse item rows, added as INTEGERS (fixed-point terms, 2^-30), then one
// correctly rounded fp64 divide and one rounding to fp32 per token; a score is a fixed fp32 fma chain over the item's
// own tokens in storage order.  So no result depends on how the work is dealt to lanes, waves or workgroups, or on the
// order the atomics land in.
//   k_content  one workgroup per list.
//     profile  groups of kContentGroup = 8 lanes take the history entries g, g + 32, ...; the lanes of a group stride
//              the tokens of the entry's item row (a categorical row holds about 8) and add llrint(w * x * 2^30) as
//              int64.  Lane 0 of a group sums llrint(|w| * 2^30), one 64-bit LDS atomic per group at the end.
//     image    p[v] = (float)((double)P[v] / (double)Wq).
//     scores   thread j, j + 256, ... walks item j's tokens from 0: acc = fma(p[tok], x, acc).
//   Three forms, by where the sums and the image live (the score phase reads the image once per token slot of the whole
//   item CSR, the profile phase touches the sums once per slot of the history's rows alone, so the image is what LDS
//   is worth most to):
//     0  n_tokens * 8 bytes fit kContentLdsBytes (18432 tokens): the sums in LDS, the image written over the low word of
//        a token's own int64 slot: one array, no second one.
//     1  n_tokens * 4 bytes fit (36864 tokens: a synopsis vocabulary): the sums on the list's row of the workspace
//        (zeroed by the call, 64-bit global atomics, read back past the L1), the image in LDS.
//     2  above: sums and image on the workspace row, the image in place as in form 0, read past the L1.
#include <hip/hip_runtime.h>
#include <math.h>

#include "anirec_dev.hpp"

namespace anirec {

constexpr size_t kContentLdsBytes = 147456;  // 144 KiB of int64 sums: n_tokens <= 18432 accumulate in LDS
constexpr int kContentGroup = 8;             // lanes that share one history entry
constexpr double kContentScale = 1073741824.0;  // 2^30
constexpr double kContentMaxTerm = 1024.0;

struct ContentArgs {
  const int64_t *tok_offsets;  // [n_items + 1]
  const int32_t *tok_idx;
  const float *tok_w;
  int n_items, n_tokens;
  const int32_t *offsets;  // [n_lists + 1]
  const int32_t *hist_idx;
  const float *hist_w;     // optional
  int n_hist;
  float *out;              // [n_lists][n_items]
  unsigned long long *S;   // global form: [n_lists][n_tokens], zeroed by the call; LDS form: unused
  int32_t *err;
};

template <int kForm>
__global__ __launch_bounds__(256) void k_content(ContentArgs a) {
  constexpr bool kLds = kForm == 0;  // the sums are in LDS
  extern __shared__ unsigned long long content_sum[];
  float *img = (float *)content_sum;  // form 0: slot v's low word is img[2 v]; form 1: img[v]
  __shared__ unsigned long long wq_sum;
  const int tid = threadIdx.x;
  const size_t l = blockIdx.x;
  float *out = a.out + l * (size_t)a.n_items;
  const int lo = a.offsets[l], hi = a.offsets[l + 1];
  if (lo < 0 || hi < lo || hi > a.n_hist) {  // a bad pair: the row is NaN, nothing is read through it
    if (tid == 0) *a.err = 1;
    for (int j = tid; j < a.n_items; j += 256) out[j] = __uint_as_float(0x7FC00000u);
    return;
  }
  unsigned long long *S = kLds ? content_sum : a.S + l * (size_t)a.n_tokens;
  if (kLds)
    for (int v = tid; v < a.n_tokens; v += 256) S[v] = 0ull;
  if (tid == 0) wq_sum = 0ull;
  __syncthreads();

  bool bad = false;
  const int g = tid / kContentGroup, gl = tid % kContentGroup;
  long long wq = 0;
  for (long long e = (long long)lo + g; e < hi; e += 256 / kContentGroup) {
    const int i = a.hist_idx[e];
    const double w = a.hist_w ? (double)a.hist_w[e] : 1.0;
    if ((uint32_t)i >= (uint32_t)a.n_items || !(fabs(w) <= kContentMaxTerm)) {  // the entry adds nothing, to Wq either
      bad = true;
      continue;
    }
    if (gl == 0) wq += llrint(fabs(w) * kContentScale);
    const int64_t t1 = a.tok_offsets[i + 1];
    for (int64_t t = a.tok_offsets[i] + gl; t < t1; t += kContentGroup) {
      const int v = a.tok_idx[t];
      if ((uint32_t)v >= (uint32_t)a.n_tokens) {
        bad = true;
        continue;
      }
      const double prod = w * (double)a.tok_w[t];  // exact: two 24-bit significands
      if (!(fabs(prod) <= kContentMaxTerm)) {      // NaN, an infinite factor or a term past the documented range
        bad = true;
        continue;
      }
      const long long term = llrint(prod * kContentScale);  // an exact scaling, rounded to the nearest even integer
      if (term) atomicAdd(&S[v], (unsigned long long)term);
    }
  }
  if (wq) atomicAdd(&wq_sum, (unsigned long long)wq);
  __syncthreads();

  {
#pragma clang fp contract(off)
    const long long Wq = (long long)wq_sum;
    const double dw = (double)Wq;
    for (int v = tid; v < a.n_tokens; v += 256) {
      const long long P = (long long)(kLds ? S[v] : __hip_atomic_load(&S[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      const float p = Wq > 0 ? (float)__ddiv_rn((double)P, dw) : 0.0f;
      // forms 0 and 2: the fp32 image takes the low word of the token's own slot, which no other thread touches in
      // this phase
      if (kForm == 0)
        img[2 * v] = p;
      else if (kForm == 1)
        img[v] = p;
      else
        __hip_atomic_store((uint32_t *)&S[v], __float_as_uint(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();

  for (int j = tid; j < a.n_items; j += 256) {
    const int64_t t1 = a.tok_offsets[j + 1];
    float acc = 0.0f;
    for (int64_t t = a.tok_offsets[j]; t < t1; ++t) {  // storage order: the chain is part of the rule
      const int v = a.tok_idx[t];
      const float x = a.tok_w[t];
      if ((uint32_t)v >= (uint32_t)a.n_tokens || !(fabsf(x) <= 3.40282346638528859812e+38f)) {
        bad = true;
        continue;
      }
      const float p = kForm == 0   ? img[2 * v]
                      : kForm == 1 ? img[v]
                                   : __uint_as_float(__hip_atomic_load((const uint32_t *)&S[v], __ATOMIC_RELAXED,
                                                                       __HIP_MEMORY_SCOPE_AGENT));
      acc = __fmaf_rn(p, x, acc);
    }
    out[j] = acc;
  }
  if (bad) *a.err = 1;
}

static bool content_in_lds(int32_t n_tokens) { return (size_t)n_tokens * 8 <= kContentLdsBytes; }
static bool content_image_in_lds(int32_t n_tokens) { return (size_t)n_tokens * 4 <= kContentLdsBytes; }

}  // namespace anirec

using namespace anirec;

extern "C" {

size_t anirec_content_lds_tokens(void) { return kContentLdsBytes / 8; }

size_t anirec_content_workspace_bytes(int32_t n_tokens, int32_t n_lists) {
  if (n_tokens < 1 || n_lists < 0) return 0;
  if (content_in_lds(n_tokens) || n_lists == 0) return 256;
  return (size_t)n_lists * (size_t)n_tokens * 8;
}

int anirec_content_scores(const int64_t *tok_offsets, const int32_t *tok_idx, const float *tok_w, int32_t n_items,
                          int32_t n_tokens, const int32_t *hist_offsets, const int32_t *hist_idx, const float *hist_w,
                          int32_t n_lists, int32_t n_hist, float *out_scores, int32_t *err_flag, void *ws,
                          size_t ws_bytes, void *stream) {
  if (n_items < 1 || n_tokens < 1 || n_lists < 0 || n_hist < 0) return ANIREC_EINVAL;
  if (n_lists == 0) return ANIREC_OK;
  if (!tok_offsets || !tok_idx || !tok_w || !hist_offsets || !out_scores || !err_flag || !ws ||
      (n_hist > 0 && !hist_idx))
    return ANIREC_EINVAL;
  if (ws_bytes < anirec_content_workspace_bytes(n_tokens, n_lists)) return ANIREC_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  ContentArgs a;
  a.tok_offsets = tok_offsets;
  a.tok_idx = tok_idx;
  a.tok_w = tok_w;
  a.n_items = n_items;
  a.n_tokens = n_tokens;
  a.offsets = hist_offsets;
  a.hist_idx = hist_idx;
  a.hist_w = hist_w;
  a.n_hist = n_hist;
  a.out = out_scores;
  a.S = (unsigned long long *)ws;
  a.err = err_flag;
  if (content_in_lds(n_tokens)) {
    ANIREC_HIP_CHECK(hipFuncSetAttribute((const void *)k_content<0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)kContentLdsBytes));
    hipLaunchKernelGGL(k_content<0>, dim3(n_lists), dim3(256), (size_t)n_tokens * 8, s, a);
    return (int)hipGetLastError();
  }
  ANIREC_HIP_CHECK(hipMemsetAsync(ws, 0, (size_t)n_lists * (size_t)n_tokens * 8, s));
  if (content_image_in_lds(n_tokens)) {
    ANIREC_HIP_CHECK(hipFuncSetAttribute((const void *)k_content<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)kContentLdsBytes));
    hipLaunchKernelGGL(k_content<1>, dim3(n_lists), dim3(256), (size_t)n_tokens * 4, s, a);
  } else {
    hipLaunchKernelGGL(k_content<2>, dim3(n_lists), dim3(256), 0, s, a);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
