// Implicit-feedback ALS for gfx950 (MI355X): the Gram matrix of a factor table and one conjugate-gradient half-sweep
// (include/anirec.h, anirec_als_gram / anirec_als_half_sweep).
//
// A half-sweep refits every row of one table with the other table Y frozen.  The fits of different rows share nothing
// but Y and G = Y^T Y, so a call is one launch:
//   k_als_sweep  one workgroup of 256 lanes per row, k_fold_in's shape: a row is one float4 per lane of a group of
//                kG = width / 4 lanes, the workgroup holds kNG = 256 / kG groups, EVERY group keeps x, r, p in registers
//                (identical copies).  The operator A v = G v + lambda v + sum_i e_i (y_i . v) y_i is never formed: one
//                walk gives every group a partial float4 of it,
//                  rows g, g + kNG, ... of G:      acc += v[k] * G[k][cols]     (G is symmetric: column sums by rows)
//                  entries g, g + kNG, ... of I:   acc += (e_i * (y_i . v)) * y_i,  y_i . v by the group butterfly
//                and the kNG partials meet in LDS, every lane adding its column in group order 0 .. kNG-1.  The scalar
//                products of CG (r.r, p.Ap) are group butterflies over identical copies.  No atomics; the order
//                depends on the row's list length and the width alone, so a row's bits do not depend on the other rows,
//                its position, `order` or the run.
// G and the Y rows are not staged: they come through L2 (G is 4 .. 256 KB; at width 256 it exceeds the CU's 160 KB LDS
// and at 128 it would hold a CU to two workgroups), so every width and list length takes the one path.
// LDS: 256 float4 partials + kNG loss partials + one row of scalars (5.1 KB at most).
//
//   k_gram_part  G's partial sums over chunks of ANIREC_ALS_GRAM_CHUNK rows: every product of two floats is taken in
//                fp64 (exact) and added in row order; k_gram_sum adds a cell's chunk partials in chunk order and rounds
//                once to fp32.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>

#include "anirec_dev.hpp"

namespace anirec {

struct AlsArgs {
  const float *Y;          // [n_other][dim] the frozen table
  int n_other;
  const float *G;          // [dim][dim] Y^T Y
  const int64_t *offsets;  // [n_rows + 1]
  const int32_t *idx;
  const float *excess;     // optional: NULL means alpha for every entry
  float alpha;
  const int32_t *order;    // optional [n_rows]: workgroup b takes row order[b]
  float *X;                // [n_rows][dim], refitted in place
  int n_rows;
  float lambda;
  int cg_steps;
  float *row_loss;         // [n_rows]
  int32_t *err;
};

__device__ __forceinline__ float dot4(const float4 &a, const float4 &b) {
#pragma clang fp contract(off)
  return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
}

// Nothing in this kernel is contracted: every product and every sum is rounded once, in the order written, so that the
// NumPy restatement (tests/als_restatement.py) is the same arithmetic.
template <int kD>
__global__ __launch_bounds__(256) void k_als_sweep(AlsArgs a) {
#pragma clang fp contract(off)
  constexpr int kG = kD / 4, kNG = 256 / kG;
  __shared__ __attribute__((aligned(16))) float4 red[256];  // [kNG][kG]: the groups' partial rows
  __shared__ float lred[kNG];                               // the groups' partial loss sums
  __shared__ __attribute__((aligned(16))) float vs[kD];     // the vector A is applied to, as scalars
  const int tid = threadIdx.x, l = tid & (kG - 1), g = tid / kG;
  const float qnan = __uint_as_float(0x7FC00000u);
  int row = blockIdx.x;
  if (a.order) {
    row = a.order[blockIdx.x];
    if ((uint32_t)row >= (uint32_t)a.n_rows) {  // no row to poison: the flag alone
      if (tid == 0) *a.err = 1;
      return;
    }
  }
  float4 *x4 = reinterpret_cast<float4 *>(a.X) + (size_t)row * kG;
  const long long lo = a.offsets[row], hi = a.offsets[row + 1];
  const bool bad_range = lo < 0 || hi < lo || hi - lo > (long long)INT_MAX;
  if (!bad_range && hi == lo) {  // an empty list: the minimiser is 0 exactly
    if (g == 0) x4[l] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid == 0) a.row_loss[row] = 0.f;
    return;
  }
  // nothing is read through a bad offset pair or a bad index: the whole list is checked before any row is gathered
  const int n = bad_range ? 0 : (int)(hi - lo);
  const int32_t *ix = a.idx + (bad_range ? 0 : lo);
  const float *ex = a.excess ? a.excess + (bad_range ? 0 : lo) : nullptr;
  int bad = bad_range ? 1 : 0;
  for (int i = tid; i < n; i += 256) bad |= ((uint32_t)ix[i] >= (uint32_t)a.n_other) ? 1 : 0;
  if (__syncthreads_or(bad)) {
    if (g == 0) x4[l] = make_float4(qnan, qnan, qnan, qnan);
    if (tid == 0) {
      a.row_loss[row] = qnan;
      *a.err = 1;
    }
    return;
  }
  const float4 *Y4 = reinterpret_cast<const float4 *>(a.Y);
  const float4 *G4 = reinterpret_cast<const float4 *>(a.G);
  const float lam = a.lambda;

  // kMode 0: A v without the lambda term.  1: sum_i ((1 + e_i) - e_i (y_i . v)) y_i - G v (the residual at v without
  // its lambda term).  2: G v, and lt = sum_i (1 + e_i)(1 - s_i)^2 - s_i^2 with s_i = y_i . v.
  // Every lane of every group returns the same total.
  auto walk = [&](auto mode, const float4 &v, float &lt) -> float4 {
    constexpr int kMode = decltype(mode)::value;
    if (g == 0) reinterpret_cast<float4 *>(vs)[l] = v;
    __syncthreads();
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float lsum = 0.f;
    for (int k = g; k < kD; k += kNG) {
      const float4 q = G4[k * kG + l];
      const float w = kMode == 1 ? -vs[k] : vs[k];
      acc.x += w * q.x;
      acc.y += w * q.y;
      acc.z += w * q.z;
      acc.w += w * q.w;
    }
    for (int i = g; i < n; i += kNG) {
      const float4 y = Y4[(size_t)ix[i] * kG + l];
      const float e = ex ? ex[i] : a.alpha;
      const float s = group_sum<kG>(dot4(y, v));
      if (kMode == 2) {
        const float d = 1.0f - s;
        lsum += (1.0f + e) * (d * d) - s * s;
      } else {
        const float c = kMode == 1 ? (1.0f + e) - e * s : e * s;
        acc.x += c * y.x;
        acc.y += c * y.y;
        acc.z += c * y.z;
        acc.w += c * y.w;
      }
    }
    red[tid] = acc;
    if (kMode == 2 && l == 0) lred[g] = lsum;
    __syncthreads();
    float4 t = red[l];
    lt = kMode == 2 ? lred[0] : 0.f;
#pragma unroll 4
    for (int k = 1; k < kNG; ++k) {  // fixed order: group 0, 1, ..., the same in every group
      const float4 q = red[k * kG + l];
      t.x += q.x;
      t.y += q.y;
      t.z += q.z;
      t.w += q.w;
      if (kMode == 2) lt += lred[k];
    }
    __syncthreads();  // red / lred / vs are rewritten by the next walk
    return t;
  };

  float4 x = x4[l];
  float unused;
  if (a.cg_steps > 0) {
    float4 r = walk(std::integral_constant<int, 1>(), x, unused);
    r.x -= lam * x.x;
    r.y -= lam * x.y;
    r.z -= lam * x.z;
    r.w -= lam * x.w;
    float4 p = r;
    float rs = group_sum<kG>(dot4(r, r));
    const float floor_rs = ANIREC_ALS_CG_RTOL2 * rs;
    for (int t = 0; t < a.cg_steps; ++t) {  // rs is the same bits in every lane: the exit is uniform
      if (!(rs > floor_rs)) break;
      float4 Ap = walk(std::integral_constant<int, 0>(), p, unused);
      Ap.x += lam * p.x;
      Ap.y += lam * p.y;
      Ap.z += lam * p.z;
      Ap.w += lam * p.w;
      const float al = rs / group_sum<kG>(dot4(p, Ap));
      x.x += al * p.x;
      x.y += al * p.y;
      x.z += al * p.z;
      x.w += al * p.w;
      r.x -= al * Ap.x;
      r.y -= al * Ap.y;
      r.z -= al * Ap.z;
      r.w -= al * Ap.w;
      const float rsn = group_sum<kG>(dot4(r, r));
      const float be = rsn / rs;
      p.x = r.x + be * p.x;
      p.y = r.y + be * p.y;
      p.z = r.z + be * p.z;
      p.w = r.w + be * p.w;
      rs = rsn;
    }
  }
  float lt;
  const float4 Gx = walk(std::integral_constant<int, 2>(), x, lt);
  const float xGx = group_sum<kG>(dot4(x, Gx));
  const float xx = group_sum<kG>(dot4(x, x));
  if (g == 0) x4[l] = x;
  if (tid == 0) a.row_loss[row] = (xGx + lt) + lam * xx;
}

// ---- G = Y^T Y ------------------------------------------------------------------------------------------------------
constexpr int kGramChunk = ANIREC_ALS_GRAM_CHUNK;
constexpr int kGramStage = 32;  // rows staged in LDS at a time

// grid (n_chunks, tiles_a * tiles_b): a workgroup owns a kT x kT tile of G (kT = min(kD, 64)) over one chunk of rows;
// thread (i, j) of a 16 x 16 grid owns kT/16 x kT/16 cells.  part: [n_chunks][kD][kD] fp64.
template <int kD>
__global__ __launch_bounds__(256) void k_gram_part(const float *Y, int n, double *part) {
  constexpr int kT = kD < 64 ? kD : 64, kR = kT / 16, kTiles = kD / kT;
  __shared__ float As[kGramStage][kT];
  __shared__ float Bs[kGramStage][kT];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int c = blockIdx.x, ta = blockIdx.y / kTiles, tb = blockIdx.y % kTiles;
  const long long r0 = (long long)c * kGramChunk;
  const int rows = (int)min((long long)kGramChunk, (long long)n - r0);
  double acc[kR][kR];
#pragma unroll
  for (int i = 0; i < kR; ++i)
#pragma unroll
    for (int j = 0; j < kR; ++j) acc[i][j] = 0.0;
  for (int s0 = 0; s0 < rows; s0 += kGramStage) {
    if (s0) __syncthreads();  // the previous rows have been read
    for (int e = tid; e < kGramStage * kT; e += 256) {
      const int r = e / kT, col = e % kT;
      float av = 0.f, bv = 0.f;  // rows past the chunk's end add exact zeros
      if (s0 + r < rows) {
        const float *y = Y + (size_t)(r0 + s0 + r) * kD;
        av = y[ta * kT + col];
        bv = y[tb * kT + col];
      }
      As[r][col] = av;
      Bs[r][col] = bv;
    }
    __syncthreads();
    for (int r = 0; r < kGramStage; ++r) {  // row order: the sum of a cell over a chunk is one fixed chain
#pragma unroll
      for (int i = 0; i < kR; ++i)
#pragma unroll
        for (int j = 0; j < kR; ++j) acc[i][j] += (double)As[r][ti * kR + i] * (double)Bs[r][tj * kR + j];
    }
  }
  double *out = part + (size_t)c * kD * kD;
#pragma unroll
  for (int i = 0; i < kR; ++i)
#pragma unroll
    for (int j = 0; j < kR; ++j) out[(size_t)(ta * kT + ti * kR + i) * kD + tb * kT + tj * kR + j] = acc[i][j];
}

__global__ __launch_bounds__(256) void k_gram_sum(const double *part, int n_chunks, int cells, float *G) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= cells) return;
  double s = part[e];
  for (int c = 1; c < n_chunks; ++c) s += part[(size_t)c * cells + e];  // fixed order: chunk 0, 1, ...
  G[e] = (float)s;
}

static size_t gram_chunks(int32_t n) { return ((size_t)n + kGramChunk - 1) / kGramChunk; }

}  // namespace anirec

using namespace anirec;

extern "C" {

size_t anirec_als_gram_workspace_bytes(int32_t n, int32_t dim) {
  if (n < 1 || !dim_ok(dim)) return 0;
  return gram_chunks(n) * (size_t)dim * (size_t)dim * sizeof(double);
}

int anirec_als_gram(const float *Y, int32_t n, int32_t dim, float *G_out, void *workspace, size_t workspace_bytes,
                    void *stream) {
  if (!dim_ok(dim) || n < 1 || !Y || !G_out || !workspace || ((uintptr_t)workspace & 7)) return ANIREC_EINVAL;
  if (workspace_bytes < anirec_als_gram_workspace_bytes(n, dim)) return ANIREC_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int n_chunks = (int)gram_chunks(n);
  double *part = (double *)workspace;
  with_width(dim, [&](auto kd) {
    constexpr int kD = decltype(kd)::value;
    constexpr int kTiles = kD / (kD < 64 ? kD : 64);
    hipLaunchKernelGGL(k_gram_part<kD>, dim3((unsigned)n_chunks, kTiles * kTiles), dim3(256), 0, s, Y, n, part);
  });
  const int cells = dim * dim;
  hipLaunchKernelGGL(k_gram_sum, dim3((cells + 255) / 256), dim3(256), 0, s, part, n_chunks, cells, G_out);
  return (int)hipGetLastError();
}

int anirec_als_half_sweep(const float *Y, int32_t n_other, int32_t dim, const float *G, const int64_t *offsets,
                          const int32_t *idx, const float *excess, float alpha, const int32_t *order, float *X_inout,
                          int32_t n_rows, float lambda, int32_t cg_steps, float *row_loss, int32_t *err_flag,
                          void *stream) {
  if (!dim_ok(dim) || n_other < 1 || n_rows < 0 || cg_steps < 0 || cg_steps > ANIREC_ALS_MAX_CG) return ANIREC_EINVAL;
  if (!(lambda >= 0.f) || !(lambda <= FLT_MAX) || !(alpha >= 0.f) || !(alpha <= FLT_MAX)) return ANIREC_EINVAL;
  if (n_rows == 0) return ANIREC_OK;
  if (!Y || !G || !offsets || !X_inout || !row_loss || !err_flag) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  AlsArgs a;
  a.Y = Y;
  a.n_other = n_other;
  a.G = G;
  a.offsets = offsets;
  a.idx = idx;
  a.excess = excess;
  a.alpha = alpha;
  a.order = order;
  a.X = X_inout;
  a.n_rows = n_rows;
  a.lambda = lambda;
  a.cg_steps = cg_steps;
  a.row_loss = row_loss;
  a.err = err_flag;
  with_width(dim, [&](auto kd) {
    hipLaunchKernelGGL(k_als_sweep<decltype(kd)::value>, dim3((unsigned)n_rows), dim3(256), 0, s, a);
  });
  return (int)hipGetLastError();
}

}  // extern "C"
