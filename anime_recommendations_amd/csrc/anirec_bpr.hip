// Bayesian Personalised Ranking matrix factorisation (Rendle et al. 2009) for gfx950 (MI355X): SGD over sampled
// (user, liked item, unliked item) triples (include/anirec.h, anirec_bpr_steps / anirec_bpr_sample).
//
// Everything that crosses a lane group is an INTEGER: the sampler is a counter-based hash of (seed, step, slot), the
// gradient of a step is summed per (row, column) as int64 of 2^30-scaled fp32 terms, the rows' slot counts are int32.
// So a step's result does not depend on how the slots are dealt to lanes, waves or workgroups, nor on the order the
// atomics land in, and a NumPy restatement (tests/bpr_restatement.py) is the same bits.
//
// A step is two launches over the batch's slots, a group of kG = width / 4 lanes (one float4 each, k_als_sweep's row
// shape) per slot, 256 / kG slots per workgroup pass:
//   k_bpr_grad   draws the slot's triple (every lane of the group the same draw: the loads are broadcasts), keeps it in
//                the workspace for the apply phase, reads x_u, y_i, y_j, takes x^ by the group butterfly, the stated
//                sigmoid, and adds the three rows' fixed-point terms with 64-bit integer atomics.  The accumulator of a
//                row is laid out [4][kG] (component-major), so one wave-instruction adds kG consecutive int64 per row:
//                64 .. 512 contiguous bytes.  It reads the tables and writes accumulators only.
//   k_bpr_apply  walks the same slots; for each of a slot's three rows one lane exchanges the row's count with 0, and
//                the group that receives a count > 0 (exactly one per touched row) applies the update and returns the
//                row's accumulators to zero.  No table is scanned; the tables are written here only.
// No kernel waits on another workgroup; all launches of a call are enqueued at once.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>

#include "anirec_dev.hpp"

namespace anirec {

constexpr int kBprMaxTries = ANIREC_BPR_MAX_TRIES;
constexpr int kBprBlocks = 4096;  // the most workgroups of a phase: the groups stride over the slots

struct BprArgs {
  float *X;                // [n_users][F]
  float *Y;                // [n_items][F]
  int n_users, n_items;
  const int64_t *offsets;  // [n_users + 1]
  const int32_t *idx;      // [nnz]
  const int32_t *pair_user;  // [nnz]
  uint32_t nnz;
  int batch, tries;
  uint32_t seed, step;
  float lr, reg;
  int bias;
  unsigned long long *acc_x;  // [n_users][4][kG] fixed-point sums
  unsigned long long *acc_y;  // [n_items][4][kG]
  int32_t *cnt_x;             // [n_users] slots touching the row
  int32_t *cnt_y;             // [n_items]
  int32_t *trip;              // [batch][3] the step's triples
  unsigned long long *counts; // [3] of this step: kept, dropped, x^ > 0
  int32_t *err;
};

__device__ __forceinline__ uint32_t bpr_mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ uint32_t bpr_pick(uint32_t r, uint32_t n) { return __umulhi(r, n); }

// The triple of (step t, slot s): 0 = kept, 1 = dropped (j = -1), 2 = an index out of range (u = i = j = -1, nothing
// read through it).  Every loop is bounded by tries and 32 halvings.
__device__ __forceinline__ int bpr_draw(const int64_t *__restrict__ offsets, const int32_t *__restrict__ idx,
                                        const int32_t *__restrict__ pair_user, int n_users, int n_items, uint32_t nnz,
                                        int tries, uint32_t seed, uint32_t t, uint32_t s, int &u, int &i, int &j) {
  const uint32_t h = bpr_mix32(bpr_mix32(seed + 0x9e3779b9u * t) ^ bpr_mix32(s + 0x85ebca6bu));
  const uint32_t p = bpr_pick(bpr_mix32(h + 0x9e3779b9u), nnz);
  u = pair_user[p];
  i = idx[p];
  j = -1;
  if ((uint32_t)u >= (uint32_t)n_users || (uint32_t)i >= (uint32_t)n_items) {
    u = i = -1;
    return 2;
  }
  const long long lo = offsets[u], hi = offsets[u + 1];
  if (lo < 0 || hi < lo || hi > (long long)nnz) {
    u = i = -1;
    return 2;
  }
  for (int c = 1; c <= tries; ++c) {
    const int cand = (int)bpr_pick(bpr_mix32(h + 0x9e3779b9u * (uint32_t)(c + 1)), (uint32_t)n_items);
    long long a = lo, b = hi;  // the first entry >= cand of the ascending row
    while (a < b) {
      const long long m = a + ((b - a) >> 1);
      if (idx[m] < cand) a = m + 1; else b = m;
    }
    if (a == hi || idx[a] != cand) {
      j = cand;
      return 0;
    }
  }
  return 1;
}

// 1 / (1 + e(x)), e the stated exponential: no library transcendental, every operation rounded once
__device__ __forceinline__ float bpr_sigmoid_neg(float x) {
#pragma clang fp contract(off)
  const float xc = fminf(fmaxf(x, -30.0f), 30.0f);  // a NaN becomes -30
  const float kf = rintf(xc * 1.44269502162933349609375f);
  const float r = (xc - kf * 0.693145751953125f) - kf * 1.428606765330187045037746429443359375e-06f;
  float p = 1.38888892251998186111450195312e-03f;   // 1/720
  p = p * r + 8.33333376795053482055664062500e-03f;  // 1/120
  p = p * r + 4.16666679084300994873046875000e-02f;  // 1/24
  p = p * r + 1.66666671633720397949218750000e-01f;  // 1/6
  p = p * r + 0.5f;
  p = p * r + 1.0f;
  p = p * r + 1.0f;
  const float e = ldexpf(p, (int)kf);
  return 1.0f / (1.0f + e);
}

// the fixed-point term of one fp32 product; a value that is not finite or above 2^20 in magnitude adds 0 and flags
__device__ __forceinline__ long long bpr_term(float v, bool &diverged) {
  if (!(fabsf(v) <= 1048576.0f)) {
    diverged = true;
    return 0ll;
  }
  return llrint((double)v * 1073741824.0);
}

__device__ __forceinline__ float bpr_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

template <int kG>
__device__ __forceinline__ void bpr_add_row(unsigned long long *acc, int l, long long t0, long long t1, long long t2,
                                            long long t3) {
  if (t0) atomicAdd(acc + l, (unsigned long long)t0);
  if (t1) atomicAdd(acc + kG + l, (unsigned long long)t1);
  if (t2) atomicAdd(acc + 2 * kG + l, (unsigned long long)t2);
  if (t3) atomicAdd(acc + 3 * kG + l, (unsigned long long)t3);
}

template <int kD>
__global__ __launch_bounds__(256) void k_bpr_grad(BprArgs a) {
#pragma clang fp contract(off)
  constexpr int kG = kD / 4, kNG = 256 / kG;
  const int tid = threadIdx.x, l = tid & (kG - 1), g = tid / kG;
  const float4 *X4 = reinterpret_cast<const float4 *>(a.X);
  const float4 *Y4 = reinterpret_cast<const float4 *>(a.Y);
  unsigned long long kept = 0, dropped = 0, positive = 0;
  bool bad = false, diverged = false;
  for (long long s = (long long)blockIdx.x * kNG + g; s < a.batch; s += (long long)gridDim.x * kNG) {
    int u, i, j;
    const int st = bpr_draw(a.offsets, a.idx, a.pair_user, a.n_users, a.n_items, a.nnz, a.tries, a.seed, a.step,
                            (uint32_t)s, u, i, j);
    if (l == 0) {
      a.trip[3 * s] = u;
      a.trip[3 * s + 1] = i;
      a.trip[3 * s + 2] = j;
    }
    if (st != 0) {
      bad = bad || st == 2;
      dropped += 1;
      continue;
    }
    kept += 1;
    const float4 x = X4[(size_t)u * kG + l];
    const float4 yi = Y4[(size_t)i * kG + l], yj = Y4[(size_t)j * kG + l];
    const float4 d = make_float4(yi.x - yj.x, yi.y - yj.y, yi.z - yj.z, yi.w - yj.w);
    const float xh = group_sum<kG>(((x.x * d.x + x.y * d.y) + x.z * d.z) + x.w * d.w);
    if (xh > 0.0f) positive += 1;
    const float gs = bpr_sigmoid_neg(xh);
    const long long u0 = bpr_term(bpr_mul(gs, d.x), diverged), u1 = bpr_term(bpr_mul(gs, d.y), diverged);
    const long long u2 = bpr_term(bpr_mul(gs, d.z), diverged), u3 = bpr_term(bpr_mul(gs, d.w), diverged);
    const long long v0 = bpr_term(bpr_mul(gs, x.x), diverged), v1 = bpr_term(bpr_mul(gs, x.y), diverged);
    const long long v2 = bpr_term(bpr_mul(gs, x.z), diverged), v3 = bpr_term(bpr_mul(gs, x.w), diverged);
    bpr_add_row<kG>(a.acc_x + (size_t)u * kD, l, u0, u1, u2, u3);
    bpr_add_row<kG>(a.acc_y + (size_t)i * kD, l, v0, v1, v2, v3);
    bpr_add_row<kG>(a.acc_y + (size_t)j * kD, l, -v0, -v1, -v2, -v3);
    if (l == 0) {
      atomicAdd(a.cnt_x + u, 1);
      atomicAdd(a.cnt_y + i, 1);
      atomicAdd(a.cnt_y + j, 1);
    }
  }
  if (l == 0) {
    if (kept) atomicAdd(a.counts, kept);
    if (dropped) atomicAdd(a.counts + 1, dropped);
    if (positive) atomicAdd(a.counts + 2, positive);
  }
  if (bad) atomicOr(a.err, ANIREC_BPR_ERR_INDEX);
  if (diverged) atomicOr(a.err, ANIREC_BPR_ERR_DIVERGED);
}

// one row's update by the group that won its count c > 0; skip_last: column kD - 1 keeps its value (a user row's 1)
template <int kD>
__device__ __forceinline__ void bpr_apply_row(float *table, unsigned long long *acc, int row, int l, int c, float lr,
                                              float reg, bool skip_last) {
#pragma clang fp contract(off)
  constexpr int kG = kD / 4;
  float4 *x4 = reinterpret_cast<float4 *>(table) + (size_t)row * kG + l;
  unsigned long long *ar = acc + (size_t)row * kD;
  const float4 x = *x4;
  const float xs[4] = {x.x, x.y, x.z, x.w};
  float out[4];
  const float rc = reg * (float)c;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long sum = (long long)ar[k * kG + l];
    ar[k * kG + l] = 0ull;
    const float grad = (float)((double)sum * 9.31322574615478515625e-10);  // 2^-30
    out[k] = xs[k] + lr * (grad - rc * xs[k]);
  }
  if (skip_last && l == kG - 1) out[3] = xs[3];
  *x4 = make_float4(out[0], out[1], out[2], out[3]);
}

template <int kD>
__global__ __launch_bounds__(256) void k_bpr_apply(BprArgs a) {
  constexpr int kG = kD / 4, kNG = 256 / kG;
  const int tid = threadIdx.x, l = tid & (kG - 1), g = tid / kG;
  for (long long s = (long long)blockIdx.x * kNG + g; s < a.batch; s += (long long)gridDim.x * kNG) {
    const int u = a.trip[3 * s], i = a.trip[3 * s + 1], j = a.trip[3 * s + 2];
    if (j < 0) continue;  // dropped, or an index out of range: the slot touched nothing
    int cu = 0, ci = 0, cj = 0;
    if (l == 0) {
      cu = atomicExch(a.cnt_x + u, 0);
      ci = atomicExch(a.cnt_y + i, 0);
      cj = atomicExch(a.cnt_y + j, 0);
    }
    cu = __shfl(cu, 0, kG);
    ci = __shfl(ci, 0, kG);
    cj = __shfl(cj, 0, kG);
    if (cu > 0) bpr_apply_row<kD>(a.X, a.acc_x, u, l, cu, a.lr, a.reg, a.bias != 0);
    if (ci > 0) bpr_apply_row<kD>(a.Y, a.acc_y, i, l, ci, a.lr, a.reg, false);
    if (cj > 0) bpr_apply_row<kD>(a.Y, a.acc_y, j, l, cj, a.lr, a.reg, false);
  }
}

__global__ __launch_bounds__(256) void k_bpr_sample(const int64_t *__restrict__ offsets, const int32_t *__restrict__ idx,
                                                    const int32_t *__restrict__ pair_user, int n_users, int n_items,
                                                    uint32_t nnz, int batch, int tries, uint32_t seed, uint32_t step0,
                                                    int n_steps, int32_t *__restrict__ out, int32_t *__restrict__ err) {
  const size_t total = (size_t)n_steps * (size_t)batch;
  bool bad = false;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const uint32_t t = step0 + (uint32_t)(e / (size_t)batch), s = (uint32_t)(e % (size_t)batch);
    int u, i, j;
    bad = (bpr_draw(offsets, idx, pair_user, n_users, n_items, nnz, tries, seed, t, s, u, i, j) == 2) || bad;
    out[3 * e] = u;
    out[3 * e + 1] = i;
    out[3 * e + 2] = j;
  }
  if (bad) atomicOr(err, ANIREC_BPR_ERR_INDEX);
}

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// the workspace: [acc_x | acc_y | cnt_x | cnt_y] (zeroed by the call, zero again after every step) then [trip]
struct BprLayout {
  size_t acc_x, acc_y, cnt_x, cnt_y, zeroed, trip, total;
};

static BprLayout bpr_layout(int32_t n_users, int32_t n_items, int32_t width, int32_t batch) {
  BprLayout w;
  w.acc_x = 0;
  w.acc_y = w.acc_x + up256((size_t)n_users * (size_t)width * 8);
  w.cnt_x = w.acc_y + up256((size_t)n_items * (size_t)width * 8);
  w.cnt_y = w.cnt_x + up256((size_t)n_users * 4);
  w.zeroed = w.cnt_y + up256((size_t)n_items * 4);
  w.trip = w.zeroed;
  w.total = w.trip + up256((size_t)batch * 12);
  return w;
}

static bool bpr_sampler_ok(int32_t n_users, int32_t n_items, int64_t nnz, int32_t batch, int32_t tries, int32_t step0,
                           int32_t n_steps) {
  return n_users >= 1 && n_items >= 1 && nnz >= 1 && nnz < (1ll << 31) && batch >= 1 && tries >= 1 &&
         tries <= kBprMaxTries && step0 >= 0 && n_steps >= 0 && (long long)step0 + (long long)n_steps <= (long long)INT_MAX;
}

}  // namespace anirec

using namespace anirec;

extern "C" {

size_t anirec_bpr_workspace_bytes(int32_t n_users, int32_t n_items, int32_t width, int32_t batch) {
  if (n_users < 1 || n_items < 1 || !dim_ok(width) || batch < 1) return 0;
  return bpr_layout(n_users, n_items, width, batch).total;
}

int anirec_bpr_sample(const int64_t *offsets, const int32_t *idx, const int32_t *pair_user, int32_t n_users,
                      int32_t n_items, int64_t nnz, int32_t batch, int32_t tries, uint32_t seed, int32_t step0,
                      int32_t n_steps, int32_t *out_triples, int32_t *err_flag, void *stream) {
  if (!bpr_sampler_ok(n_users, n_items, nnz, batch, tries, step0, n_steps)) return ANIREC_EINVAL;
  if (!offsets || !idx || !pair_user || !err_flag || (n_steps > 0 && !out_triples)) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  if (n_steps == 0) return ANIREC_OK;
  const size_t total = (size_t)n_steps * (size_t)batch, blocks = (total + 255) / 256;
  hipLaunchKernelGGL(k_bpr_sample, dim3((unsigned)(blocks > 65536 ? 65536 : blocks)), dim3(256), 0, s, offsets, idx,
                     pair_user, n_users, n_items, (uint32_t)nnz, batch, tries, seed, (uint32_t)step0, n_steps,
                     out_triples, err_flag);
  return (int)hipGetLastError();
}

int anirec_bpr_steps(float *X, float *Y, int32_t n_users, int32_t n_items, int32_t width, const int64_t *offsets,
                     const int32_t *idx, const int32_t *pair_user, int64_t nnz, int32_t batch, int32_t tries,
                     uint32_t seed, int32_t step0, int32_t n_steps, float lr, float reg, int32_t bias,
                     int64_t *out_counts, int32_t *err_flag, void *ws, size_t ws_bytes, void *stream) {
  if (!dim_ok(width) || !bpr_sampler_ok(n_users, n_items, nnz, batch, tries, step0, n_steps)) return ANIREC_EINVAL;
  if (!(lr >= 0.f) || !(lr <= FLT_MAX) || !(reg >= 0.f) || !(reg <= FLT_MAX) || (bias != 0 && bias != 1))
    return ANIREC_EINVAL;
  if (!X || !Y || !offsets || !idx || !pair_user || !err_flag || !ws || (n_steps > 0 && !out_counts))
    return ANIREC_EINVAL;
  if ((((uintptr_t)X | (uintptr_t)Y) & 15) || (((uintptr_t)ws | (uintptr_t)out_counts) & 7)) return ANIREC_EINVAL;
  const BprLayout w = bpr_layout(n_users, n_items, width, batch);
  if (ws_bytes < w.total) return ANIREC_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  if (n_steps == 0) return ANIREC_OK;
  char *base = (char *)ws;
  ANIREC_HIP_CHECK(hipMemsetAsync(base, 0, w.zeroed, s));
  ANIREC_HIP_CHECK(hipMemsetAsync(out_counts, 0, (size_t)n_steps * 3 * 8, s));
  BprArgs a;
  a.X = X;
  a.Y = Y;
  a.n_users = n_users;
  a.n_items = n_items;
  a.offsets = offsets;
  a.idx = idx;
  a.pair_user = pair_user;
  a.nnz = (uint32_t)nnz;
  a.batch = batch;
  a.tries = tries;
  a.seed = seed;
  a.lr = lr;
  a.reg = reg;
  a.bias = bias;
  a.acc_x = (unsigned long long *)(base + w.acc_x);
  a.acc_y = (unsigned long long *)(base + w.acc_y);
  a.cnt_x = (int32_t *)(base + w.cnt_x);
  a.cnt_y = (int32_t *)(base + w.cnt_y);
  a.trip = (int32_t *)(base + w.trip);
  a.err = err_flag;
  with_width(width, [&](auto kd) {
    constexpr int kD = decltype(kd)::value;
    constexpr int kNG = 1024 / kD;
    const long long want = ((long long)batch + kNG - 1) / kNG;
    const dim3 grid((unsigned)(want > kBprBlocks ? kBprBlocks : want));
    for (int t = 0; t < n_steps; ++t) {
      a.step = (uint32_t)step0 + (uint32_t)t;
      a.counts = (unsigned long long *)out_counts + (size_t)t * 3;
      hipLaunchKernelGGL(k_bpr_grad<kD>, grid, dim3(256), 0, s, a);
      hipLaunchKernelGGL(k_bpr_apply<kD>, grid, dim3(256), 0, s, a);
    }
  });
  return (int)hipGetLastError();
}

}  // extern "C"
