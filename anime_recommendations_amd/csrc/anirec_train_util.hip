// Utilities beside libanirec's training path for gfx950 (MI355X): the flat optimiser steps with an explicit gradient,
// the rating gather, and the self-tests of the lazy replay's square root and divide, each with its entry point.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "anirec_train_lazy.hpp"

namespace anirec {

// flat Adam with an explicit gradient (unit-testable bit-exact stage)
__global__ __launch_bounds__(256) void k_adam_flat(float *w, float *m, float *v, const float *g,
                                                   size_t n, float alpha) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float ww = w[i], mm = m[i], vv = v[i];
    adam_elem(ww, mm, vv, g[i], alpha);
    w[i] = ww;
    m[i] = mm;
    v[i] = vv;
  }
}

// flat one-slot update with an explicit gradient (anirec_opt_flat; the dense kernel's element rule)
template <int kOpt>
__global__ __launch_bounds__(256) void k_opt_flat(float *w, float *slot, const float *g, size_t n, float rate) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float ww = w[i], mm = 0.f, vv = kOpt == ANIREC_OPT_SGD ? 0.f : slot[i];
    opt_elem<kOpt>(ww, mm, vv, g[i], rate);
    w[i] = ww;
    if (kOpt != ANIREC_OPT_SGD) slot[i] = vv;
  }
}

// Self-test of the lazy replay's short sequences (anirec_selftest_lazy_math; tests only).  Square root: EVERY float
// of the range the sequence is used on, [2^-96, 2^96], against the compiler's correctly rounded sqrtf — 1.6 x 10^9
// inputs, exhaustive.  Divide: `n_div` pseudo-random (numerator, denominator) pairs drawn over the ranges the
// replay admits, against the IEEE `/` (the sequence is the compiler's own Markstein chain without its scaling and
// fix-up steps, so this is a regression guard, not the argument).  counts[0] += sqrt mismatches, counts[1] += divide
// mismatches.
template <int kVar>
__global__ __launch_bounds__(256) void k_selftest_lazy_math(unsigned long long n_div, unsigned long long *counts) {
  const unsigned long long tid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long nth = (unsigned long long)gridDim.x * blockDim.x;
  const uint32_t lo = __float_as_uint(0x1p-96f), hi = __float_as_uint(0x1p96f);
  unsigned long long bad_s = 0, bad_d = 0;
  for (unsigned long long b = (unsigned long long)lo + 4 * tid; b <= hi; b += 4 * nth) {
    Quad x;
    x.a.x = __uint_as_float((uint32_t)min(b + 0, (unsigned long long)hi));
    x.a.y = __uint_as_float((uint32_t)min(b + 1, (unsigned long long)hi));
    x.b.x = __uint_as_float((uint32_t)min(b + 2, (unsigned long long)hi));
    x.b.y = __uint_as_float((uint32_t)min(b + 3, (unsigned long long)hi));
    const Quad s = sqrt4_normal<kVar>(x);
    bad_s += __float_as_uint(s.a.x) != __float_as_uint(sqrtf(x.a.x));
    bad_s += __float_as_uint(s.a.y) != __float_as_uint(sqrtf(x.a.y));
    bad_s += __float_as_uint(s.b.x) != __float_as_uint(sqrtf(x.b.x));
    bad_s += __float_as_uint(s.b.y) != __float_as_uint(sqrtf(x.b.y));
  }
  // numerators +-[2^-60, 2^60], denominators [1e-7, 2^48]: mantissa bits and exponent from a 64-bit mix of the index
  auto mix = [](unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  auto draw = [&](unsigned long long h, int e_lo, int e_span, bool sign) {
    const uint32_t man = (uint32_t)h & 0x7FFFFFu;
    const uint32_t ex = (uint32_t)(127 + e_lo + (int)((h >> 23) % (unsigned)e_span));
    const uint32_t sg = sign ? (uint32_t)((h >> 40) & 1u) << 31 : 0u;
    return __uint_as_float(sg | (ex << 23) | man);
  };
  for (unsigned long long i = 4 * tid; i < n_div; i += 4 * nth) {
    float nv[4], dv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned long long h1 = mix(2 * (i + k)), h2 = mix(2 * (i + k) + 1);
      nv[k] = draw(h1, -60, 120, true);
      dv[k] = fmaxf(draw(h2, -24, 72, false), kAdamEps);
    }
    const Quad n = {{nv[0], nv[1]}, {nv[2], nv[3]}}, d = {{dv[0], dv[1]}, {dv[2], dv[3]}};
    const Quad q = div4_normal(n, d);
    const float qs[4] = {q.a.x, q.a.y, q.b.x, q.b.y};
#pragma unroll
    for (int k = 0; k < 4; ++k) bad_d += __float_as_uint(qs[k]) != __float_as_uint(nv[k] / dv[k]);
  }
  bad_s = (unsigned long long)wave_sum_d((double)bad_s);
  bad_d = (unsigned long long)wave_sum_d((double)bad_d);
  if ((threadIdx.x & 63) == 0) {
    if (bad_s) atomicAdd(counts + 0, bad_s);
    if (bad_d) atomicAdd(counts + 1, bad_d);
  }
}

// Self-test of the replay's one-correction divide (anirec_selftest_lazy_div; tests only), see div4_normal.
// kMode 0: the refined reciprocal against 1.0f / d on EVERY float d with bits in [lo, hi].  kMode 1: q1 against the
// IEEE `/` on every significand pair n, d in [1, 2), d's significands [lo, hi) (one workgroup each) x all 2^23 n's.
// kMode 2: the same with the uncorrected q0 = n y (the comparison's own sanity leg: it must report misses).
// counts[0] += mismatches, counts[1] += operands checked, counts[2] / counts[3] = min / max bits of a failing d.
template <int kMode>
__global__ __launch_bounds__(256) void k_selftest_lazy_div(uint32_t lo, uint32_t hi, unsigned long long *counts) {
  unsigned long long bad = 0, seen = 0;
  uint32_t fmin = 0xFFFFFFFFu, fmax = 0u;
  if (kMode == 0) {
    const unsigned long long tid = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long nth = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long b = (unsigned long long)lo + 4 * tid; b <= hi; b += 4 * nth) {
      uint32_t u[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) u[k] = (uint32_t)min(b + k, (unsigned long long)hi);
      const Quad d = {{__uint_as_float(u[0]), __uint_as_float(u[1])}, {__uint_as_float(u[2]), __uint_as_float(u[3])}};
      const Quad y = rcp4_refined(d);
      const float ys[4] = {y.a.x, y.a.y, y.b.x, y.b.y};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (b + k > hi) continue;
        ++seen;
        if (__float_as_uint(ys[k]) != __float_as_uint(1.0f / __uint_as_float(u[k]))) {
          ++bad;
          fmin = min(fmin, u[k]);
          fmax = max(fmax, u[k]);
        }
      }
    }
  } else {
    const uint32_t db = 0x3F800000u | (lo + blockIdx.x);
    const float dv = __uint_as_float(db);
    const Quad d = {{dv, dv}, {dv, dv}};
    for (uint32_t i = 4 * threadIdx.x; i < (1u << 23); i += 4 * blockDim.x) {
      const Quad n = {{__uint_as_float(0x3F800000u | i), __uint_as_float(0x3F800000u | (i + 1))},
                      {__uint_as_float(0x3F800000u | (i + 2)), __uint_as_float(0x3F800000u | (i + 3))}};
      Quad q;
      if (kMode == 1) {
        q = div4_normal(n, d);
      } else {
        const Quad y = rcp4_refined(d);
        q = n * y;
      }
      const float qs[4] = {q.a.x, q.a.y, q.b.x, q.b.y}, ns[4] = {n.a.x, n.a.y, n.b.x, n.b.y};
#pragma unroll
      for (int k = 0; k < 4; ++k) bad += __float_as_uint(qs[k]) != __float_as_uint(ns[k] / dv);
      seen += 4;
    }
    if (bad) fmin = fmax = db;
  }
  bad = (unsigned long long)wave_sum_d((double)bad);
  seen = (unsigned long long)wave_sum_d((double)seen);
  if ((threadIdx.x & 63) == 0) {
    if (bad) atomicAdd(counts + 0, bad);
    atomicAdd(counts + 1, seen);
  }
  if (fmin != 0xFFFFFFFFu) {
    atomicMin(counts + 2, (unsigned long long)fmin);
    atomicMax(counts + 3, (unsigned long long)fmax);
  }
}

__global__ __launch_bounds__(256) void k_gather_ratings(const int32_t *ui, const int32_t *ai,
                                                        const float *t, const int64_t *perm,
                                                        size_t n, int32_t *uo, int32_t *ao,
                                                        float *to) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t p = perm[i];
    uo[i] = ui[p];
    ao[i] = ai[p];
    to[i] = t[p];
  }
}

}  // namespace anirec

using namespace anirec;

extern "C" {

int anirec_adam_flat(float *w, float *m, float *v, const float *g, size_t n, float alpha,
                     void *stream) {
  if (!w || !m || !v || !g) return ANIREC_EINVAL;
  if (n == 0) return ANIREC_OK;
  size_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_adam_flat, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, m,
                     v, g, n, alpha);
  return (int)hipGetLastError();
}

int anirec_opt_flat(int32_t kind, float *w, float *slot, const float *g, size_t n, float rate, void *stream) {
  if (kind < ANIREC_OPT_SGD || kind > ANIREC_OPT_ADAGRAD || !w || !g || (kind != ANIREC_OPT_SGD && !slot))
    return ANIREC_EINVAL;
  if (n == 0) return ANIREC_OK;
  size_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipStream_t s = (hipStream_t)stream;
  if (kind == ANIREC_OPT_SGD)
    hipLaunchKernelGGL(k_opt_flat<ANIREC_OPT_SGD>, dim3((unsigned)blocks), dim3(256), 0, s, w, slot, g, n, rate);
  else if (kind == ANIREC_OPT_RMSPROP)
    hipLaunchKernelGGL(k_opt_flat<ANIREC_OPT_RMSPROP>, dim3((unsigned)blocks), dim3(256), 0, s, w, slot, g, n, rate);
  else
    hipLaunchKernelGGL(k_opt_flat<ANIREC_OPT_ADAGRAD>, dim3((unsigned)blocks), dim3(256), 0, s, w, slot, g, n, rate);
  return (int)hipGetLastError();
}

int anirec_selftest_lazy_math(uint64_t n_div, uint64_t *counts2, void *stream) {
  if (!counts2) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(counts2, 0, 2 * sizeof(uint64_t), s));
  // ANIREC_SELFTEST_NEWTON=0|2 (the test's own sanity legs): the square root without its Newton correction (only
  // faithful: the comparison must report misses) / with a second one, instead of the ONE the replay uses
  const char *var = getenv("ANIREC_SELFTEST_NEWTON");
  const int steps = var && (var[0] == '0' || var[0] == '2') ? var[0] - '0' : 1;
  if (steps == 0)
    hipLaunchKernelGGL(k_selftest_lazy_math<0>, dim3(8192), dim3(256), 0, s, (unsigned long long)n_div,
                       reinterpret_cast<unsigned long long *>(counts2));
  else if (steps == 2)
    hipLaunchKernelGGL(k_selftest_lazy_math<2>, dim3(8192), dim3(256), 0, s, (unsigned long long)n_div,
                       reinterpret_cast<unsigned long long *>(counts2));
  else
    hipLaunchKernelGGL(k_selftest_lazy_math<1>, dim3(8192), dim3(256), 0, s, (unsigned long long)n_div,
                       reinterpret_cast<unsigned long long *>(counts2));
  return (int)hipGetLastError();
}

int anirec_selftest_lazy_div(int32_t mode, uint32_t lo, uint32_t hi, uint64_t *counts4, void *stream) {
  if (!counts4 || mode < 0 || mode > 2 || hi < lo) return ANIREC_EINVAL;
  if (mode != 0 && hi > (1u << 23)) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const uint64_t init[4] = {0, 0, ~0ull, 0};
  ANIREC_HIP_CHECK(hipMemcpyAsync(counts4, init, sizeof(init), hipMemcpyHostToDevice, s));
  ANIREC_HIP_CHECK(hipStreamSynchronize(s));  // (init lives on this stack frame)
  unsigned long long *c = reinterpret_cast<unsigned long long *>(counts4);
  if (mode == 0) {
    hipLaunchKernelGGL(k_selftest_lazy_div<0>, dim3(8192), dim3(256), 0, s, lo, hi, c);
  } else if (hi > lo) {
    if (mode == 1)
      hipLaunchKernelGGL(k_selftest_lazy_div<1>, dim3(hi - lo), dim3(256), 0, s, lo, hi, c);
    else
      hipLaunchKernelGGL(k_selftest_lazy_div<2>, dim3(hi - lo), dim3(256), 0, s, lo, hi, c);
  }
  return (int)hipGetLastError();
}

int anirec_gather_ratings(const int32_t *user_in, const int32_t *anime_in, const float *rating_in,
                          const int64_t *perm, size_t n, int32_t *user_out, int32_t *anime_out,
                          float *rating_out, void *stream) {
  if (!user_in || !anime_in || !rating_in || !perm || !user_out || !anime_out || !rating_out)
    return ANIREC_EINVAL;
  if (n == 0) return ANIREC_OK;
  size_t blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(k_gather_ratings, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     user_in, anime_in, rating_in, perm, n, user_out, anime_out, rating_out);
  return (int)hipGetLastError();
}

}  // extern "C"
