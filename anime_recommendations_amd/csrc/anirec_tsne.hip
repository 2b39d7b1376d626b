// Exact t-SNE on an embedding table's neighbour graph, for gfx950 (MI355X): include/anirec.h, anirec_tsne_forces /
// anirec_tsne_fit.  All pairs in two dimensions, exact and order-free: a pair term is a fixed fp32 chain (nothing
// contracted) quantised to an INTEGER (rint(p * 2^30), |p| <= 1), a row's force is an int64 sum of those, the
// normaliser Z a two-word (128-bit) sum of them, and the update of a row is a chain of correctly rounded fp64
// operations — so no result depends on lanes, waves, j_splits or the order the atomics land in.
//   forces   k_tsne_forces: a lane owns one i point and its three int64 sums (Z part, Rx, Ry) in registers; the j points
//            of the workgroup's j range are staged in LDS anirec_tsne_tile() = 1024 float2 at a time and every lane
//            reads the SAME float2 (an LDS broadcast, no bank conflicts).  A row that is out (a coordinate not finite or
//            above 2^60) is staged as a far sentinel, whose chain gives exactly 0 for every term; a tile is padded to a
//            multiple of 4 with the same sentinel.  The self pair runs through the chain like any other (dx = dy = 0:
//            q = 1, force 0) and its 2^30 is taken off Z once a row — no compare in the loop.  grid.y = j_splits ranges
//            of j; Rx / Ry partials land by 64-bit integer atomicAdd on SoA arrays (consecutive lanes, consecutive
//            8-byte words), the workgroup's Z part by one two-word add (low word atomicAdd, a carry into the high word
//            by whoever wrapped it).
//   attract  k_tsne_attract: 16 lanes a row walk the row's stored pairs (a hub row of n - 1 entries is 1/16 of that a
//            lane), the integer partials meet by shuffles, and lane 0 of the 16 either writes Ax / Ay (forces call) or
//            runs the row's fp64 update (fit), which also zeroes the row's Rx / Ry for the next iteration.
// A fit is one init kernel, then iters x (forces, attract + update), all plain launches enqueued at once.  Y is double
// buffered (an update must not move a point another row still reads): iteration t reads buffer (iters - t) & 1 and
// writes the other, buffer 0 being Y_inout, so the last iteration writes Y_inout; with an odd iters the init kernel
// copies Y_inout to buffer 1 first.  Z has a slot of its own per iteration: nothing is reset while another workgroup may
// read it.  Workspace: float2 Ybuf [n], int64 Rx [n], Ry [n], uint64 Z [iters][2]; zeroed by the init kernel.
#include <hip/hip_runtime.h>
#include <math.h>

#include "anirec_dev.hpp"

namespace anirec {

constexpr int kTsThreads = 256;
constexpr int kTsTile = 1024;           // float2 j points of one LDS tile
constexpr int kTsRowLanes = 16;         // attract: lanes that share a row
constexpr int kTsMaxSplits = 1024;
constexpr int kTsTargetBlocks = 1024;   // the library's j_splits: about this many workgroups
constexpr float kTsScale = 1073741824.f;   // 2^30
constexpr float kTsMaxCoord = 1152921504606846976.f;  // 2^60: a usable coordinate
constexpr float kTsFar = 3.0e38f;       // the sentinel: (x - far)^2 = inf for every usable x, so q = 0 and 0 * dx = 0

typedef unsigned long long ull;

static_assert(kTsTile % 4 == 0, "a tile is padded to a multiple of 4");
static_assert(kTsThreads % kTsRowLanes == 0 && 64 % kTsRowLanes == 0, "a row's lanes lie in one wave");

__device__ __forceinline__ bool ts_usable(float2 p) { return fabsf(p.x) <= kTsMaxCoord && fabsf(p.y) <= kTsMaxCoord; }

// rint(p * 2^30) of |p| < 2: the product is exact, one rounding to the nearest even integer, inside int32
__device__ __forceinline__ int ts_q(float p) {
#pragma clang fp contract(off)
  const float s = p * kTsScale;
  return __float2int_rn(s);
}

// the two-word sum: v < 2^63 into {low, high}
__device__ __forceinline__ void ts_add128(ull *z, ull v) {
  const ull old = atomicAdd(z, v);
  if (old + v < old) atomicAdd(z + 1, 1ull);
}

__global__ __launch_bounds__(kTsThreads) void k_tsne_forces(const float2 *Y, int n, int len, ull *Rx, ull *Ry, ull *Z,
                                                            int32_t *info) {
#pragma clang fp contract(off)
  __shared__ float2 tile[kTsTile];
  __shared__ long long zpart[kTsThreads / 64];
  const int g = threadIdx.x;
  const long long j0 = (long long)blockIdx.y * len;
  if (j0 >= n) return;  // the whole workgroup: a range past the end
  const int j1 = (int)min((long long)n, j0 + len);
  const long long i = (long long)blockIdx.x * kTsThreads + g;
  const bool live = i < n;
  float2 p = live ? Y[i] : make_float2(0.f, 0.f);
  const bool ok = live && ts_usable(p);
  if (!ok) p = make_float2(0.f, 0.f);  // a stand-in: the sums of such a lane go nowhere
  if (live && !ok && blockIdx.y == 0) atomicOr(info, 1);
  long long z = 0, rx = 0, ry = 0;
  for (int base = (int)j0; base < j1; base += kTsTile) {
    const int tc = min(kTsTile, j1 - base), tc4 = (tc + 3) & ~3;
    __syncthreads();  // the tile before is done with
    for (int e = g; e < tc4; e += kTsThreads) {
      float2 v = make_float2(kTsFar, kTsFar);
      if (e < tc) {
        const float2 y = Y[base + e];
        if (ts_usable(y)) v = y;
      }
      tile[e] = v;
    }
    __syncthreads();
    // Four pairs a step, their terms met in 32 bits first: I(q) <= 2^30, so two of them fit a uint32; |I(w dx)| <
    // 2^28.5, so four of them fit an int32.  Sums of integers: the grouping cannot change a bit, and a step has four
    // 64-bit adds instead of twelve.
    for (int jj = 0; jj < tc4; jj += 4) {
      int iq[4], ix[4], iy[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float2 b = tile[jj + u];
        const float dx = p.x - b.x, dy = p.y - b.y;
        const float xx = dx * dx, yy = dy * dy;
        const float d2 = xx + yy;
        const float q = __fdiv_rn(1.f, 1.f + d2);
        const float w = q * q;
        iq[u] = ts_q(q);
        ix[u] = ts_q(w * dx);
        iy[u] = ts_q(w * dy);
      }
      z += (long long)((unsigned)iq[0] + (unsigned)iq[1]) + (long long)((unsigned)iq[2] + (unsigned)iq[3]);
      rx += (long long)((ix[0] + ix[1]) + (ix[2] + ix[3]));
      ry += (long long)((iy[0] + iy[1]) + (iy[2] + iy[3]));
    }
  }
  if (ok && i >= j0 && i < j1) z -= 1ll << 30;  // the self pair: q = 1, no force
  if (!ok) z = 0;
  if (ok) {
    if (rx) atomicAdd(Rx + i, (ull)rx);
    if (ry) atomicAdd(Ry + i, (ull)ry);
  }
  for (int s = 32; s > 0; s >>= 1) z += __shfl_xor(z, s);
  if ((g & 63) == 0) zpart[g >> 6] = z;
  __syncthreads();
  if (g == 0) {
    long long t = 0;
    for (int w = 0; w < kTsThreads / 64; ++w) t += zpart[w];
    if (t) ts_add128(Z, (ull)t);  // t >= 0: every term is
  }
}

struct TsAttrArgs {
  const float2 *Y;         // the coordinates this iteration reads
  float2 *Ynext;           // update: the coordinates it writes
  int n;
  const int64_t *offsets;  // [n + 1]
  const int32_t *idx;
  const float *val;
  long long nnz;
  ull *Rx, *Ry;            // update: read, then zeroed
  const ull *Z;            // update: this iteration's {low, high}
  long long *Ax, *Ay;      // forces call: the outputs
  double *V, *G;           // update: [n][2]
  double e, mom, lr;       // update: exaggeration of this iteration, momentum, learning rate
  int32_t *info;
};

__device__ __forceinline__ int ts_sgn(double x) { return (int)(x > 0.0) - (int)(x < 0.0); }

// one coordinate of a row's update: gradient, gain, velocity; returns the new coordinate.  Plain operators under
// contract(off): each is one correctly rounded fp64 operation and none can fuse with its neighbour.
__device__ __forceinline__ float ts_step(float y, long long A, long long R, double zd, double den_a, const TsAttrArgs &a,
                                         double *v_io, double *g_io) {
#pragma clang fp contract(off)
  const double ea = a.e * (double)A;
  const double att = ea / den_a;
  const double rep = zd > 0.0 ? (double)R / zd : 0.0;
  const double diff = att - rep;
  const double grad = 4.0 * diff;
  double v = *v_io, gn = *g_io;
  gn = ts_sgn(grad) != ts_sgn(v) ? gn + 0.2 : gn * 0.8;
  if (gn < 0.01) gn = 0.01;
  const double mv = a.mom * v, lg = a.lr * gn;
  const double step = lg * grad;
  v = mv - step;
  *v_io = v;
  *g_io = gn;
  const double yn = (double)y + v;
  return (float)yn;
}

template <bool kUpdate>
__global__ __launch_bounds__(kTsThreads) void k_tsne_attract(TsAttrArgs a) {
#pragma clang fp contract(off)
  const int g = threadIdx.x, sub = g & (kTsRowLanes - 1);
  const long long i = ((long long)blockIdx.x * kTsThreads + g) / kTsRowLanes;
  const bool live = i < a.n;
  float2 p = make_float2(0.f, 0.f);
  bool ok = false;
  long long b = 0, e = 0;
  int bits = 0;
  if (live) {
    p = a.Y[i];
    ok = ts_usable(p);
    b = a.offsets[i];
    e = a.offsets[i + 1];
    if (b < 0 || e > a.nnz || b > e) {  // not a list inside idx / val: the row has no stored pairs
      bits |= 4;
      e = b = 0;
    }
    if (!ok) e = b;
  }
  long long ax = 0, ay = 0;
  for (long long t = b + sub; t < e; t += kTsRowLanes) {
    const int32_t j = a.idx[t];
    const float v = a.val[t];
    if ((unsigned)j >= (unsigned)a.n || j == i) {
      bits |= 4;
      continue;
    }
    if (!(v >= 0.f && v <= 2.f)) {
      bits |= 2;
      continue;
    }
    const float2 o = a.Y[j];
    if (!ts_usable(o)) continue;  // (the forces kernel has raised bit 0 for that row)
    const float dx = p.x - o.x, dy = p.y - o.y;
    const float xx = dx * dx, yy = dy * dy;
    const float d2 = xx + yy;
    const float q = __fdiv_rn(1.f, 1.f + d2);
    const float w = v * q;
    ax += ts_q(w * dx);
    ay += ts_q(w * dy);
  }
  for (int s = kTsRowLanes / 2; s > 0; s >>= 1) {
    ax += __shfl_xor(ax, s);
    ay += __shfl_xor(ay, s);
    bits |= __shfl_xor(bits, s);
  }
  if (!live || sub) return;
  if (bits) atomicOr(a.info, bits);
  if constexpr (!kUpdate) {
    a.Ax[i] = ax;
    a.Ay[i] = ay;
  } else {
    const long long rx = (long long)a.Rx[i], ry = (long long)a.Ry[i];
    a.Rx[i] = 0;
    a.Ry[i] = 0;
    const double zhi = (double)a.Z[1] * 18446744073709551616.0;
    const double zd = zhi + (double)a.Z[0];
    const double den_a = 2147483648.0 * (double)a.n;  // 2 n 2^30, exact
    double *V = a.V + 2 * i, *G = a.G + 2 * i;
    float2 out;  // (p as it is: a row that is out has sums of 0 and moves by its velocity alone)
    out.x = ts_step(p.x, ax, rx, zd, den_a, a, V, G);
    out.y = ts_step(p.y, ay, ry, zd, den_a, a, V + 1, G + 1);
    a.Ynext[i] = out;
  }
}

// the first kernel of either call: every accumulator and flag to zero; fit: V = 0, G = 1, and Y into the second buffer
__global__ __launch_bounds__(kTsThreads) void k_tsne_init(ull *w0, size_t n0, ull *w1, size_t n1, ull *w2, size_t n2,
                                                          int32_t *info, double *V, double *G, const float2 *Y, float2 *Ycopy,
                                                          int n) {
  const size_t stride = (size_t)gridDim.x * kTsThreads, first = (size_t)blockIdx.x * kTsThreads + threadIdx.x;
  for (size_t e = first; e < n0; e += stride) w0[e] = 0ull;
  for (size_t e = first; e < n1; e += stride) w1[e] = 0ull;
  for (size_t e = first; e < n2; e += stride) w2[e] = 0ull;
  if (first == 0) *info = 0;
  if (V) {
    for (size_t e = first; e < 2 * (size_t)n; e += stride) {
      V[e] = 0.0;
      G[e] = 1.0;
    }
  }
  if (Ycopy) {
    for (size_t e = first; e < (size_t)n; e += stride) Ycopy[e] = Y[e];
  }
}

static inline size_t ts_ws_bytes(int n, int iters) { return (size_t)n * 24 + (size_t)iters * 16; }

static inline int ts_splits(int n, int j_splits) {
  if (j_splits > 0) return j_splits;
  const int iblocks = (n + kTsThreads - 1) / kTsThreads;
  int s = (kTsTargetBlocks + iblocks - 1) / iblocks;
  const int most = (n + 63) / 64;  // a range of fewer than 64 j points is all staging
  if (s > most) s = most;
  return s < 1 ? 1 : s;
}

static inline bool ts_args_ok(int32_t n, int32_t j_splits, int64_t nnz, const void *offsets, const void *idx,
                              const void *val) {
  if (n < 1 || n > ANIREC_TSNE_MAX_ROWS || j_splits < 0 || j_splits > kTsMaxSplits || nnz < 0) return false;
  if (!offsets || (nnz > 0 && (!idx || !val))) return false;
  return true;
}

static void ts_launch_forces(const float2 *Y, int n, int j_splits, ull *Rx, ull *Ry, ull *Z, int32_t *info, hipStream_t s) {
  const int splits = ts_splits(n, j_splits), len = (n + splits - 1) / splits;
  hipLaunchKernelGGL(k_tsne_forces, dim3((unsigned)((n + kTsThreads - 1) / kTsThreads), (unsigned)splits), dim3(kTsThreads),
                     0, s, Y, n, len, Rx, Ry, Z, info);
}

static inline unsigned ts_attr_grid(int n) {
  return (unsigned)(((long long)n * kTsRowLanes + kTsThreads - 1) / kTsThreads);
}

static inline unsigned ts_init_grid(int n) {
  const int b = (n + kTsThreads - 1) / kTsThreads;
  return (unsigned)(b < 1024 ? b : 1024);
}

}  // namespace anirec

using namespace anirec;

extern "C" {

size_t anirec_tsne_tile(void) { return kTsTile; }

size_t anirec_tsne_workspace_bytes(int32_t n_rows, int32_t iters) {
  if (n_rows < 1 || n_rows > ANIREC_TSNE_MAX_ROWS || iters < 1 || iters > ANIREC_TSNE_MAX_ITER) return 0;
  return ts_ws_bytes(n_rows, iters);
}

int anirec_tsne_forces(const float *Y, int32_t n_rows, const int64_t *offsets, const int32_t *idx, const float *val,
                       int64_t nnz, int32_t j_splits, int64_t *out_rx, int64_t *out_ry, int64_t *out_ax, int64_t *out_ay,
                       uint64_t *out_z, int32_t *out_info, void *stream) {
  if (!ts_args_ok(n_rows, j_splits, nnz, offsets, idx, val)) return ANIREC_EINVAL;
  if (!Y || !out_rx || !out_ry || !out_ax || !out_ay || !out_z || !out_info) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const float2 *Y2 = reinterpret_cast<const float2 *>(Y);
  ull *Rx = reinterpret_cast<ull *>(out_rx), *Ry = reinterpret_cast<ull *>(out_ry), *Z = reinterpret_cast<ull *>(out_z);
  hipLaunchKernelGGL(k_tsne_init, dim3(ts_init_grid(n_rows)), dim3(kTsThreads), 0, s, Rx, (size_t)n_rows, Ry,
                     (size_t)n_rows, Z, (size_t)2, out_info, (double *)nullptr, (double *)nullptr, (const float2 *)nullptr,
                     (float2 *)nullptr, n_rows);
  ts_launch_forces(Y2, n_rows, j_splits, Rx, Ry, Z, out_info, s);
  TsAttrArgs a = {};
  a.Y = Y2;
  a.n = n_rows;
  a.offsets = offsets;
  a.idx = idx;
  a.val = val;
  a.nnz = nnz;
  a.Ax = reinterpret_cast<long long *>(out_ax);
  a.Ay = reinterpret_cast<long long *>(out_ay);
  a.info = out_info;
  hipLaunchKernelGGL(k_tsne_attract<false>, dim3(ts_attr_grid(n_rows)), dim3(kTsThreads), 0, s, a);
  return (int)hipGetLastError();
}

int anirec_tsne_fit(float *Y_inout, int32_t n_rows, const int64_t *offsets, const int32_t *idx, const float *val,
                    int64_t nnz, int32_t iters, int32_t exag_iters, double exaggeration, double lr, int32_t j_splits,
                    double *out_V, double *out_G, int32_t *out_info, void *ws, size_t ws_bytes, void *stream) {
  if (!ts_args_ok(n_rows, j_splits, nnz, offsets, idx, val)) return ANIREC_EINVAL;
  if (iters < 1 || iters > ANIREC_TSNE_MAX_ITER || exag_iters < 0) return ANIREC_EINVAL;
  if (!(exaggeration > 0.0 && exaggeration <= 1e6) || !(lr > 0.0 && lr <= 1e9)) return ANIREC_EINVAL;  // (a NaN fails)
  if (!Y_inout || !out_V || !out_G || !out_info || !ws) return ANIREC_EINVAL;
  if (ws_bytes < ts_ws_bytes(n_rows, iters) || ((uintptr_t)ws & 7)) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)n_rows;
  float2 *buf[2] = {reinterpret_cast<float2 *>(Y_inout), reinterpret_cast<float2 *>(ws)};
  ull *Rx = reinterpret_cast<ull *>(ws) + n, *Ry = Rx + n, *Z = Ry + n;
  // (the whole workspace in 8-byte words: Ybuf n, Rx n, Ry n, Z 2 * iters)
  hipLaunchKernelGGL(k_tsne_init, dim3(ts_init_grid(n_rows)), dim3(kTsThreads), 0, s, reinterpret_cast<ull *>(ws),
                     3 * n + 2 * (size_t)iters, (ull *)nullptr, (size_t)0, (ull *)nullptr, (size_t)0, out_info, out_V, out_G,
                     (const float2 *)buf[0], (iters & 1) ? buf[1] : (float2 *)nullptr, n_rows);
  hipError_t e = hipGetLastError();
  TsAttrArgs a = {};
  a.n = n_rows;
  a.offsets = offsets;
  a.idx = idx;
  a.val = val;
  a.nnz = nnz;
  a.Rx = Rx;
  a.Ry = Ry;
  a.V = out_V;
  a.G = out_G;
  a.lr = lr;
  a.info = out_info;
  for (int t = 0; t < iters && e == hipSuccess; ++t) {
    const bool early = t < exag_iters;
    a.Y = buf[(iters - t) & 1];
    a.Ynext = buf[(iters - t - 1) & 1];
    a.Z = Z + 2 * (size_t)t;
    a.e = early ? exaggeration : 1.0;
    a.mom = early ? 0.5 : 0.8;
    ts_launch_forces(a.Y, n_rows, j_splits, Rx, Ry, Z + 2 * (size_t)t, out_info, s);
    hipLaunchKernelGGL(k_tsne_attract<true>, dim3(ts_attr_grid(n_rows)), dim3(kTsThreads), 0, s, a);
    e = hipGetLastError();
  }
  return (int)e;
}

}  // extern "C"
