// Hybrid lists: several systems' score rows fused into one, for gfx950 (MI355X): include/anirec.h, anirec_fuse_rows.
// Both methods are pure functions of a row's values: ranks and key extrema are integers, the fp32 steps are elementwise
// in a fixed order (system 0, 1, ...), nothing is contracted.  So no result depends on how the items are dealt to
// threads, and a NumPy restatement holds the output bit for bit.  Nothing of size [n_sys, nq, n] goes to HBM.
//   rrf     k_fuse_rrf, a workgroup per row, a dynamic LDS image of 8 n bytes (short rows leave room for several
//           workgroups a CU).  The output row is the accumulator: NaN, +0 where eligible.  Per system: the row is loaded
//           as (score_key << 32) | ~j, 0 for an item that is not eligible; lds_sort_desc (anirec_dev.hpp: the network of
//           the any-k select's k_lk_sort) sorts it; the thread that holds position r adds w / (c + 1 + r) to out[t, j].
//           Every j is touched by exactly one thread per system and a barrier separates the systems, so the adds of an
//           item happen in system order; the row is in L2 all along.
//   minmax  k_fuse_minmax, a workgroup per row, no sort: per system the largest and smallest key of the finite eligible
//           scores by wave reductions (the keys are a total order: a row holding both zeros has one answer), then one
//           pass in which a thread sums its items' terms over the systems in registers and writes each once.
// The pointers, pitches and weights of the systems travel in the argument struct; nothing is read back.
#include <hip/hip_runtime.h>

#include "anirec_dev.hpp"

namespace anirec {

constexpr uint32_t kFuseNan = 0x7FC00000u;
constexpr uint32_t kKeyPosInf = 0xFF800000u;  // score_key(+inf)
constexpr uint32_t kKeyNegInf = 0x007FFFFFu;  // score_key(-inf): the keys of the finite scores lie strictly between

struct FuseArgs {
  const float *rows[ANIREC_FUSE_MAX_SYS];  // [nq][ld] each, or [n] where ld == 0
  long long ld[ANIREC_FUSE_MAX_SYS];
  float w[ANIREC_FUSE_MAX_SYS];
  int n_sys, n;
  const uint32_t *watched;  // optional [nq][wwords]
  int wwords;
  const uint8_t *keep;      // optional [n]
  int rrf_c;
  float *out;               // [nq][ld_out]
  long long ld_out;
};

__device__ __forceinline__ bool fuse_eligible(const FuseArgs &a, const uint32_t *wrow, int j) {
  if (a.keep && !a.keep[j]) return false;
  if (wrow && ((wrow[j >> 5] >> (j & 31)) & 1u)) return false;
  return true;
}

// w / (c + 1 + r): the integer is below 2^24, so its conversion is exact; one correctly rounded division
__device__ __forceinline__ float rrf_term(float w, int c1r) {
#pragma clang fp contract(off)
  return w / (float)c1r;
}

__device__ __forceinline__ float fuse_add(float acc, float term) {
#pragma clang fp contract(off)
  return acc + term;
}

// w * v of one score under the row's extrema; span = hi - lo (0 also where the row has no finite eligible score)
__device__ __forceinline__ float minmax_term(float w, float x, float lo, float span) {
#pragma clang fp contract(off)
  float v;
  const uint32_t u = __float_as_uint(x) & 0x7FFFFFFFu;
  if (u > 0x7F800000u) {
    v = 0.f;  // NaN
  } else if (u == 0x7F800000u) {
    v = x > 0.f ? 1.f : 0.f;
  } else if (span == 0.f) {
    v = 0.f;
  } else {
    v = (x - lo) / span;
    if (v != v) v = __uint_as_float(kFuseNan);  // inf / inf where hi - lo overflows: the canonical NaN
  }
  return w * v;
}

__global__ __launch_bounds__(1024) void k_fuse_rrf(FuseArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long fuse_sw[];
  const int t = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int n = a.n;
  const uint32_t *wrow = a.watched ? a.watched + (size_t)t * a.wwords : nullptr;
  float *o = a.out + (size_t)t * (size_t)a.ld_out;
  for (int j = tid; j < n; j += nt) o[j] = fuse_eligible(a, wrow, j) ? 0.f : __uint_as_float(kFuseNan);
  for (int s = 0; s < a.n_sys; ++s) {
    const float *row = a.rows[s] + (size_t)t * (size_t)a.ld[s];
    const float w = a.w[s];
    for (int j = tid; j < n; j += nt)
      fuse_sw[j] = fuse_eligible(a, wrow, j)
                       ? ((unsigned long long)score_key(row[j]) << 32) | (unsigned long long)(~(uint32_t)j)
                       : 0ull;
    __syncthreads();  // the image is whole; on the first system, so is the accumulator row
    lds_sort_desc(fuse_sw, (uint32_t)n, tid, nt);
    for (int r = tid; r < n; r += nt) {
      const unsigned long long v = fuse_sw[r];
      if (v == 0ull) continue;  // the items that are not eligible sort behind every key
      const uint32_t j = ~(uint32_t)(v & 0xFFFFFFFFull);
      o[j] = fuse_add(o[j], rrf_term(w, a.rrf_c + 1 + r));
    }
    __syncthreads();  // this system's adds before the next one's, the image read before it is loaded again
  }
}

__global__ __launch_bounds__(1024) void k_fuse_minmax(FuseArgs a) {
  __shared__ uint32_t wmax[16], wmin[16];
  __shared__ float s_lo[ANIREC_FUSE_MAX_SYS], s_span[ANIREC_FUSE_MAX_SYS];
  const int t = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int n = a.n, nw = nt >> 6;
  const uint32_t *wrow = a.watched ? a.watched + (size_t)t * a.wwords : nullptr;
  for (int s = 0; s < a.n_sys; ++s) {
    const float *row = a.rows[s] + (size_t)t * (size_t)a.ld[s];
    uint32_t mx = 0u, mn = 0xFFFFFFFFu;
    for (int j = tid; j < n; j += nt) {
      if (!fuse_eligible(a, wrow, j)) continue;
      const uint32_t key = score_key(row[j]);
      if (key > kKeyNegInf && key < kKeyPosInf) {
        mx = key > mx ? key : mx;
        mn = key < mn ? key : mn;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const uint32_t ox = __shfl_xor(mx, off, 64), on = __shfl_xor(mn, off, 64);
      mx = ox > mx ? ox : mx;
      mn = on < mn ? on : mn;
    }
    if ((tid & 63) == 0) {
      wmax[tid >> 6] = mx;
      wmin[tid >> 6] = mn;
    }
    __syncthreads();
    if (tid == 0) {
      for (int k = 1; k < nw; ++k) {
        mx = wmax[k] > mx ? wmax[k] : mx;
        mn = wmin[k] < mn ? wmin[k] : mn;
      }
      float lo = 0.f, span = 0.f;
      if (mx != 0u) {  // a finite key is above kKeyNegInf: the row has a finite eligible score
        const float hi = __uint_as_float((mx & 0x80000000u) ? (mx ^ 0x80000000u) : ~mx);
        lo = __uint_as_float((mn & 0x80000000u) ? (mn ^ 0x80000000u) : ~mn);
        span = hi - lo;
      }
      s_lo[s] = lo;
      s_span[s] = span;
    }
    __syncthreads();  // s_lo / s_span written; wmax / wmin free for the next system
  }
  float *o = a.out + (size_t)t * (size_t)a.ld_out;
  for (int j = tid; j < n; j += nt) {
    if (!fuse_eligible(a, wrow, j)) {
      o[j] = __uint_as_float(kFuseNan);
      continue;
    }
    float acc = 0.f;
    for (int s = 0; s < a.n_sys; ++s) {
      const float x = a.rows[s][(size_t)t * (size_t)a.ld[s] + j];
      acc = fuse_add(acc, minmax_term(a.w[s], x, s_lo[s], s_span[s]));
    }
    o[j] = acc;
  }
}

}  // namespace anirec

using namespace anirec;

extern "C" {

size_t anirec_fuse_max_items(void) { return (size_t)kLdsSortMax; }

int anirec_fuse_rows(const float *const *rows_host, const int64_t *ld_host, int32_t n_sys, int32_t n, int32_t nq,
                     const uint32_t *watched, const uint8_t *keep, const float *weight_host, int32_t method,
                     int32_t rrf_c, float *out, int64_t ld_out, void *stream) {
  if (n_sys < 1 || n_sys > ANIREC_FUSE_MAX_SYS || n < 1 || n > kLdsSortMax || nq < 0) return ANIREC_EINVAL;
  if (method != ANIREC_FUSE_RRF && method != ANIREC_FUSE_MINMAX) return ANIREC_EINVAL;
  if (rrf_c < 0 || rrf_c > (1 << 20) || ld_out < (int64_t)n) return ANIREC_EINVAL;
  if (!rows_host || !ld_host || !weight_host || !out) return ANIREC_EINVAL;
  FuseArgs a;
  bool any = false;
  for (int s = 0; s < ANIREC_FUSE_MAX_SYS; ++s) {
    const bool used = s < n_sys;
    if (used) {
      const float w = weight_host[s];
      if (!rows_host[s] || (ld_host[s] != 0 && ld_host[s] < (int64_t)n)) return ANIREC_EINVAL;
      if (!(w >= 0.f && w <= 3.402823466e+38f)) return ANIREC_EINVAL;  // negative, NaN or infinite
      any = any || w > 0.f;
    }
    a.rows[s] = used ? rows_host[s] : nullptr;
    a.ld[s] = used ? (long long)ld_host[s] : 0ll;
    a.w[s] = used ? weight_host[s] : 0.f;
  }
  if (!any) return ANIREC_EINVAL;
  if (nq == 0) return ANIREC_OK;
  a.n_sys = n_sys;
  a.n = n;
  a.watched = watched;
  a.wwords = (n + 31) / 32;
  a.keep = keep;
  a.rrf_c = rrf_c;
  a.out = out;
  a.ld_out = (long long)ld_out;
  hipStream_t s = (hipStream_t)stream;
  if (method == ANIREC_FUSE_MINMAX) {
    const int nt = n >= 1024 ? 1024 : (n + 63) / 64 * 64;
    hipLaunchKernelGGL(k_fuse_minmax, dim3(nq), dim3(nt), 0, s, a);
    return (int)hipGetLastError();
  }
  ANIREC_HIP_CHECK(hipFuncSetAttribute((const void *)k_fuse_rrf, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kLdsSortMax * 8));
  uint32_t npad = 1;
  while (npad < (uint32_t)n) npad <<= 1;
  const int nt = npad / 2 < 64 ? 64 : (npad / 2 > 1024 ? 1024 : (int)(npad / 2));
  hipLaunchKernelGGL(k_fuse_rrf, dim3(nq), dim3(nt), (size_t)n * 8, s, a);
  return (int)hipGetLastError();
}

}  // extern "C"
