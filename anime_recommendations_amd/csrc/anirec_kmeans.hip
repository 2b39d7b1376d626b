// Spherical k-means on an embedding table, for gfx950 (MI355X): include/anirec.h, anirec_kmeans_assign / anirec_kmeans_fit.
// Lloyd's algorithm on the unit rows of What with the cosine as similarity, exact and order-free: a row's pick is a total
// order over k-ordered fma chains, a centroid is a sum of INTEGERS (q(x) = llrint(x * 2^30), int64) normalised in fp64,
// so no result depends on how the rows are dealt to lanes, waves or workgroups, or on the order the atomics land in.
//   assign     k_kmeans_assign: a lane owns one row, held in registers (usable = every |x| <= 2; at width 256 two lanes
//              share a row as a two-stage pipeline, see the kernel), the centroids are staged in LDS a tile of
//              anirec_kmeans_tile(dim) = 32768 / dim at a time as plain rows, and every lane reads the SAME float4
//              of a centroid pair (an LDS broadcast; the pairs interleaved float by float, so that the two chains of
//              a pair are one packed fma).  Four centroids run as four independent chains (four ds_read_b128 per 16 fmas); the pick walks the centroids in ascending c and takes a strictly larger
//              sim, so ties stay with the lowest c, across tiles as well: the running best lives in registers.  A
//              workgroup takes 256 rows at a time and keeps a one-tile image across all its rows.  In a fit the kernel
//              also counts the rows whose pick moved (per lane, one LDS atomic a lane, one global atomic a workgroup).
//   sums       k_kmeans_sums: element e = (row, t) of a workgroup's rows goes to lane e % 256: coalesced reads, and the
//              64-bit integer atomicAdds of one wave-instruction fall into 512 contiguous bytes of S[c].  Where
//              k * dim * 8 bytes fit 64 KiB the workgroup sums into LDS first (8 k rows a workgroup) and flushes its
//              non-zero partials; otherwise the adds go to global memory directly.
//   centroids  k_kmeans_centroids: one lane per centroid: the fp64 norm chain over ascending t (rounded multiply, rounded
//              add, no fma), one correctly rounded sqrt, a correctly rounded divide per element, one rounding to fp32;
//              S is zeroed for the next iteration by the lane that read it.
// A fit is max_iter x (assign, sums, centroids), one last assign, then the cluster sizes — all plain launches enqueued at
// once.  changed_j lives in a slot of its own per iteration (nothing is ever reset while another workgroup may read it);
// the centroids kernel of the iteration with changed_j == 0 raises the `done` word, and every later kernel returns on it.
// Workspace: S int64 [k][dim], then 1024 int32 {done, iterations at the stop, changed_1 .. changed_1000}; zeroed by the
// fit's first kernel, so nothing depends on what it held.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "anirec_dev.hpp"

namespace anirec {

constexpr int kKmThreads = 256;
constexpr int kKmImageFloats = 32768;   // dim * tile: the centroid image of one workgroup
constexpr int kKmChains = 4;            // centroids a lane's row meets at once
constexpr int kKmStep = 4;              // float4 of each centroid pair read ahead of the fmas that use them
constexpr int kKmMaxIter = 1000;
constexpr int kKmCtrlInts = 1024;       // done, iterations at the stop, changed_1 .. changed_kKmMaxIter
constexpr int kKmPartialBytes = 65536;  // sums: int64 partials in LDS where k * dim * 8 fits
constexpr int kKmMaxGrid = 1024;        // assign and count: workgroups that share the row batches

static_assert(2 + kKmMaxIter <= kKmCtrlInts, "one changed slot per iteration");
static_assert(ANIREC_KMEANS_MAX_K * sizeof(int) <= 65536, "the count kernel's histogram is static LDS");

struct KmAssignArgs {
  const float *What;       // [n_rows][dim] unit rows
  int n_rows;
  const float *C;          // [k][dim]
  int k, tile;
  int img_tile;            // min(k, tile): the centroids the LDS image has room for
  int32_t *out_assign;     // [n_rows]; a fit reads the previous pick from it first
  float *out_sim;          // [n_rows]
  const int32_t *done;     // fit: the stop word, or NULL
  int32_t *changed;        // fit: this iteration's slot, or NULL
};

struct KmSumsArgs {
  const float *What;
  int n_rows, k;
  const int32_t *assign;
  unsigned long long *S;   // [k][dim] int64 sums, two's complement
  const int32_t *done, *changed;
  int rows_per_block, use_lds;
};

static inline __host__ __device__ int km_tile(int dim) { return kKmImageFloats / dim; }
static inline size_t km_ws_bytes(int k, int dim) { return (size_t)k * dim * sizeof(long long) + kKmCtrlInts * sizeof(int32_t); }

// One centroid into a row's running pick: centroids arrive in ascending c, a NaN is never taken, the first pickable one
// always is, a later one only when strictly larger (so == ties, -0 and +0 among them, stay with the lowest c).
__device__ __forceinline__ void km_pick(bool in_tile, float s, int c, float &best, int &bc) {
  const bool take = in_tile & (s == s) & ((bc < 0) | (s > best));  // no branch: the four chains stay interleaved
  best = take ? s : best;
  bc = take ? c : bc;
}

// kL lanes share a row, lane `part` of them holding floats part * kH .. part * kH + kH - 1 of it (kH = kD / kL <= 128: a
// whole 256-wide row does not fit a lane's registers beside the working set).  A chain is sequential in t, so at kL = 2
// the two lanes work as a pipeline: in step s lane 0 runs the first half of the chains of centroid group s, hands the
// four running sums to lane 1 (one shuffle each), and lane 1 runs the second half of group s in step s + 1, beside lane
// 0's group s + 1: both lanes are busy in all but one step a tile.  The last lane of a row picks and writes.
template <int kD, int kL>
__global__ __launch_bounds__(kKmThreads) void k_kmeans_assign(KmAssignArgs a) {
  static_assert(kL == 1 || kL == 2, "one lane a row, or a pipeline of two");
  if (a.done && *a.done) return;
  constexpr int kRowV = kD / 4, kH = kD / kL, kHV = kH / 4, kRows = kKmThreads / kL;
  extern __shared__ __attribute__((aligned(16))) float km_smem[];
  __shared__ int moved_s;
  const int g = threadIdx.x, k = a.k, T = a.tile;
  const int part = g & (kL - 1), rl = g / kL;
  const int ntiles = (k + T - 1) / T;
  const long long nbatch = ((long long)a.n_rows + kRows - 1) / kRows;
  // the image: centroids lie in PAIRS, (c, c + 1) interleaved float by float, so that one float4 holds
  // (c[t], c+1[t], c[t+1], c+1[t+1]) and the two chains of a pair run as one packed fma with no register shuffling;
  // pair q of part p at float4 p * pstride + q * (kH / 2) + t / 2.  An odd last centroid is paired with itself.  The
  // parts lie 64 bytes askew, so that the two addresses a wave reads at once (one per part) never share a bank.
  const int pstride = ((a.img_tile + 1) / 2) * (kH / 2) + (kL > 1 ? 4 : 0);
  float4 *img = reinterpret_cast<float4 *>(km_smem);
  const float4 *mine = img + (size_t)part * pstride;
  const float4 *W4 = reinterpret_cast<const float4 *>(a.What);
  const float nanv = __uint_as_float(0x7FC00000u);
  if (g == 0) moved_s = 0;
  int moved = 0;
  bool staged = false;
  for (long long b = blockIdx.x; b < nbatch; b += gridDim.x) {
    const long long i = b * kRows + rl;
    const bool live = i < a.n_rows;
    const size_t r = (size_t)(live ? i : (long long)a.n_rows - 1);  // a lane past the end reads the last row, writes nothing
    float x[kH];
    int unusable = 0;
#pragma unroll
    for (int v = 0; v < kHV; ++v) {
      const float4 p = W4[r * kRowV + part * kHV + v];
      x[4 * v] = p.x;
      x[4 * v + 1] = p.y;
      x[4 * v + 2] = p.z;
      x[4 * v + 3] = p.w;
      // (a NaN fails <=; | not ||: no branch between the row's loads)
      unusable |= (int)!(fabsf(p.x) <= 2.f) | (int)!(fabsf(p.y) <= 2.f) | (int)!(fabsf(p.z) <= 2.f) | (int)!(fabsf(p.w) <= 2.f);
    }
    if constexpr (kL > 1) unusable |= __shfl_xor(unusable, 1);
    float best = nanv;
    int bc = -1;
    for (int tile = 0; tile < ntiles; ++tile) {
      const int base = tile * T, tc = min(T, k - base);
      if (ntiles > 1 || !staged) {
        __syncthreads();  // the chains of the tile before are done with the image
        for (int e = g; e < ((tc + 1) & ~1) * kD; e += kKmThreads) {
          const int c = e / kD, t = e - c * kD, p = t / kH, tt = t - p * kH;
          km_smem[(size_t)p * pstride * 4 + ((size_t)(c >> 1) * kH + tt) * 2 + (c & 1)] =
              a.C[(size_t)(base + min(c, tc - 1)) * kD + t];
        }
        __syncthreads();
        staged = true;
      }
      const int npairs = (tc + 1) / 2, ngroups = (npairs + 1) / 2;  // a group: two pairs, four chains
      float carry0 = 0.f, carry1 = 0.f, carry2 = 0.f, carry3 = 0.f;  // part > 0: the sums the part before has reached
      for (int step = 0; step < ngroups + kL - 1; ++step) {
        const int gi = step - part;                          // this lane's group in this step; outside 0 .. ngroups - 1:
        const bool valid = gi >= 0 && gi < ngroups;          // it runs a group again and the result goes nowhere
        const int gc = min(max(gi, 0), ngroups - 1), c0 = kKmChains * gc;
        // a last group of one pair reads that pair twice and leaves the second copy out of the pick
        const float4 *pa = mine + (size_t)(2 * gc) * (kH / 2), *pb = mine + (size_t)min(2 * gc + 1, npairs - 1) * (kH / 2);
        float s0 = part ? carry0 : 0.f, s1 = part ? carry1 : 0.f, s2 = part ? carry2 : 0.f, s3 = part ? carry3 : 0.f;
        // The row lives in registers, so the loop over t is unrolled in full; left alone the scheduler hoists every
        // LDS read of the group to the front (hundreds of registers).  So: steps of kKmStep float4 a pair, the reads of
        // the NEXT step issued before the fmas of the current one, and nothing moves across a step's end.
        float4 ya[kKmStep], yb[kKmStep], za[kKmStep], zb[kKmStep];
#pragma unroll
        for (int u = 0; u < kKmStep; ++u) {
          ya[u] = pa[u];
          yb[u] = pb[u];
        }
#pragma unroll
        for (int v0 = 0; v0 < kH / 2; v0 += kKmStep) {
          if (v0 + kKmStep < kH / 2) {
#pragma unroll
            for (int u = 0; u < kKmStep; ++u) {
              za[u] = pa[v0 + kKmStep + u];
              zb[u] = pb[v0 + kKmStep + u];
            }
          }
#pragma unroll
          for (int u = 0; u < kKmStep; ++u) {
            const int t = 2 * (v0 + u);
            s0 = __fmaf_rn(x[t], ya[u].x, s0);
            s1 = __fmaf_rn(x[t], ya[u].y, s1);
            s2 = __fmaf_rn(x[t], yb[u].x, s2);
            s3 = __fmaf_rn(x[t], yb[u].y, s3);
            s0 = __fmaf_rn(x[t + 1], ya[u].z, s0);
            s1 = __fmaf_rn(x[t + 1], ya[u].w, s1);
            s2 = __fmaf_rn(x[t + 1], yb[u].z, s2);
            s3 = __fmaf_rn(x[t + 1], yb[u].w, s3);
          }
          if (v0 + kKmStep < kH / 2) {
#pragma unroll
            for (int u = 0; u < kKmStep; ++u) {
              ya[u] = za[u];
              yb[u] = zb[u];
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (kL > 1) {  // lane 1 takes over what lane 0 has reached (lane 0 receives sums it never uses)
          carry0 = __shfl_xor(s0, 1);
          carry1 = __shfl_xor(s1, 1);
          carry2 = __shfl_xor(s2, 1);
          carry3 = __shfl_xor(s3, 1);
        }
        const bool last = valid && part == kL - 1;
        km_pick(last, s0, base + c0, best, bc);
        km_pick(last && c0 + 1 < tc, s1, base + c0 + 1, best, bc);
        km_pick(last && c0 + 2 < tc, s2, base + c0 + 2, best, bc);
        km_pick(last && c0 + 3 < tc, s3, base + c0 + 3, best, bc);
      }
    }
    if (unusable) {
      bc = -1;
      best = nanv;
    }
    if (live && part == kL - 1) {
      if (a.changed) moved += (a.out_assign[i] != bc);
      a.out_assign[i] = bc;
      a.out_sim[i] = best;
    }
  }
  if (a.changed) {
    __syncthreads();  // moved_s is zero
    if (moved) atomicAdd(&moved_s, moved);
    __syncthreads();
    if (g == 0 && moved_s) atomicAdd(a.changed, moved_s);
  }
}

// the fit's first kernel: the workspace to zero, a_0 = -2
__global__ __launch_bounds__(kKmThreads) void k_kmeans_init(unsigned long long *ws, size_t ws_words, int32_t *assign, int n_rows) {
  const size_t stride = (size_t)gridDim.x * kKmThreads;
  for (size_t e = (size_t)blockIdx.x * kKmThreads + threadIdx.x; e < ws_words; e += stride) ws[e] = 0ull;
  for (size_t e = (size_t)blockIdx.x * kKmThreads + threadIdx.x; e < (size_t)n_rows; e += stride) assign[e] = -2;
}

template <int kD>
__global__ __launch_bounds__(kKmThreads) void k_kmeans_sums(KmSumsArgs a) {
  if (*a.done || *a.changed == 0) return;
  extern __shared__ __attribute__((aligned(16))) unsigned long long km_part[];  // [k][kD] with use_lds
  const int g = threadIdx.x, kd = a.k * kD;
  const long long r0 = (long long)blockIdx.x * a.rows_per_block;
  const long long r1 = min(r0 + (long long)a.rows_per_block, (long long)a.n_rows);
  if (a.use_lds) {
    for (int e = g; e < kd; e += kKmThreads) km_part[e] = 0ull;
    __syncthreads();
  }
  for (long long e = r0 * kD + g; e < r1 * kD; e += kKmThreads) {
    const long long r = e / kD;
    const int t = (int)(e - r * kD);
    const int32_t c = a.assign[r];
    if ((unsigned)c < (unsigned)a.k) {  // -1: the row belongs to no centroid
      // q(x): the product with 2^30 is exact, one rounding to the nearest even integer
      const long long q = __double2ll_rn(__dmul_rn((double)a.What[e], 1073741824.0));
      if (a.use_lds) {
        atomicAdd(km_part + (size_t)c * kD + t, (unsigned long long)q);
      } else {
        atomicAdd(a.S + (size_t)c * kD + t, (unsigned long long)q);
      }
    }
  }
  if (a.use_lds) {
    __syncthreads();
    for (int e = g; e < kd; e += kKmThreads) {
      const unsigned long long v = km_part[e];
      if (v) atomicAdd(a.S + e, v);
    }
  }
}

// One lane per centroid.  ctrl[0] = done, ctrl[1] = the iteration of the stop; `changed` = this iteration's slot.
__global__ __launch_bounds__(64) void k_kmeans_centroids(float *C, long long *S, int k, int dim, int32_t *ctrl,
                                                         const int32_t *changed, int iter) {
#pragma clang fp contract(off)
  const bool was_done = ctrl[0] != 0;
  if (was_done || *changed == 0) {  // every lane of the launch sees the same two facts, whoever writes below
    if (!was_done && blockIdx.x == 0 && threadIdx.x == 0) {
      ctrl[1] = iter;
      ctrl[0] = 1;
    }
    return;
  }
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= k) return;
  long long *s = S + (size_t)c * dim;
  float *out = C + (size_t)c * dim;
  double nn = 0.0;
  for (int t = 0; t < dim; ++t) {
    const double d = (double)s[t];
    nn = __dadd_rn(nn, __dmul_rn(d, d));
  }
  if (nn > 0.0) {  // an empty cluster (and a sum of zeros) keeps its centroid's bits
    const double root = __dsqrt_rn(nn);
    for (int t = 0; t < dim; ++t) out[t] = (float)__ddiv_rn((double)s[t], root);
  }
  for (int t = 0; t < dim; ++t) s[t] = 0;
}

__global__ __launch_bounds__(kKmThreads) void k_kmeans_tail(const int32_t *ctrl, int max_iter, int32_t *out_info,
                                                            int32_t *out_count, int k) {
  const int e = blockIdx.x * kKmThreads + threadIdx.x;
  if (e < k) out_count[e] = 0;
  if (e == 0) {
    const int done = ctrl[0] != 0;
    out_info[0] = done ? ctrl[1] : max_iter;
    out_info[1] = done;
  }
}

__global__ __launch_bounds__(kKmThreads) void k_kmeans_count(const int32_t *assign, int n_rows, int k, int32_t *out_count) {
  __shared__ int hist[ANIREC_KMEANS_MAX_K];
  const int g = threadIdx.x;
  for (int e = g; e < k; e += kKmThreads) hist[e] = 0;
  __syncthreads();
  const long long stride = (long long)gridDim.x * kKmThreads;
  for (long long i = (long long)blockIdx.x * kKmThreads + g; i < n_rows; i += stride) {
    const int32_t c = assign[i];
    if ((unsigned)c < (unsigned)k) atomicAdd(&hist[c], 1);
  }
  __syncthreads();
  for (int e = g; e < k; e += kKmThreads) {
    const int v = hist[e];
    if (v) atomicAdd(out_count + e, v);
  }
}

static inline unsigned km_grid(int n_rows, int rows = kKmThreads) {
  const long long nbatch = ((long long)n_rows + rows - 1) / rows;
  return (unsigned)(nbatch < kKmMaxGrid ? nbatch : kKmMaxGrid);
}

template <int kD>
static hipError_t km_launch_assign(KmAssignArgs a, hipStream_t s) {
  constexpr int kL = kD > 128 ? 2 : 1;
  a.img_tile = a.k < a.tile ? a.k : a.tile;
  const size_t lds = ((size_t)((a.img_tile + 1) & ~1) * kD + (kL > 1 ? 16 * kL : 0)) * sizeof(float);
  hipError_t e = hipFuncSetAttribute((const void *)k_kmeans_assign<kD, kL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_kmeans_assign<kD, kL>), dim3(km_grid(a.n_rows, kKmThreads / kL)), dim3(kKmThreads), lds, s, a);
  return hipGetLastError();
}

}  // namespace anirec

using namespace anirec;

extern "C" {

size_t anirec_kmeans_tile(int32_t dim) { return dim_ok(dim) ? (size_t)km_tile(dim) : 0; }

size_t anirec_kmeans_workspace_bytes(int32_t n_rows, int32_t k, int32_t dim) {
  if (!dim_ok(dim) || n_rows < 1 || k < 1 || k > ANIREC_KMEANS_MAX_K) return 0;
  return km_ws_bytes(k, dim);
}

int anirec_kmeans_assign(const float *What, int32_t dim, int32_t n_rows, const float *C, int32_t k, int32_t *out_assign,
                         float *out_sim, void *stream) {
  if (!dim_ok(dim) || n_rows < 1 || k < 1 || k > ANIREC_KMEANS_MAX_K) return ANIREC_EINVAL;
  if (!What || !C || !out_assign || !out_sim) return ANIREC_EINVAL;
  KmAssignArgs a;
  a.What = What;
  a.n_rows = n_rows;
  a.C = C;
  a.k = k;
  a.tile = km_tile(dim);
  a.out_assign = out_assign;
  a.out_sim = out_sim;
  a.done = nullptr;
  a.changed = nullptr;
  int status = ANIREC_OK;
  with_width(dim, [&](auto kd) { status = (int)km_launch_assign<decltype(kd)::value>(a, (hipStream_t)stream); });
  return status;
}

int anirec_kmeans_fit(const float *What, int32_t dim, int32_t n_rows, float *C_inout, int32_t k, int32_t max_iter,
                      int32_t *out_assign, float *out_sim, int32_t *out_count, int32_t *out_info, void *ws,
                      size_t ws_bytes, void *stream) {
  if (!dim_ok(dim) || n_rows < 1 || k < 1 || k > ANIREC_KMEANS_MAX_K || max_iter < 1 || max_iter > kKmMaxIter)
    return ANIREC_EINVAL;
  if (!What || !C_inout || !out_assign || !out_sim || !out_count || !out_info || !ws) return ANIREC_EINVAL;
  if (ws_bytes < km_ws_bytes(k, dim) || ((uintptr_t)ws & 7)) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  unsigned long long *S = reinterpret_cast<unsigned long long *>(ws);
  int32_t *ctrl = reinterpret_cast<int32_t *>(S + (size_t)k * dim);
  const size_t ws_words = km_ws_bytes(k, dim) / sizeof(unsigned long long);

  KmAssignArgs a;
  a.What = What;
  a.n_rows = n_rows;
  a.C = C_inout;
  a.k = k;
  a.tile = km_tile(dim);
  a.out_assign = out_assign;
  a.out_sim = out_sim;
  a.done = ctrl;
  KmSumsArgs u;
  u.What = What;
  u.n_rows = n_rows;
  u.k = k;
  u.assign = out_assign;
  u.S = S;
  u.done = ctrl;
  u.use_lds = (size_t)k * dim * sizeof(long long) <= (size_t)kKmPartialBytes;
  u.rows_per_block = u.use_lds ? (8 * k > kKmThreads ? 8 * k : kKmThreads) : kKmThreads;
  const size_t sums_lds = u.use_lds ? (size_t)k * dim * sizeof(long long) : 0;
  const unsigned sums_grid = (unsigned)(((long long)n_rows + u.rows_per_block - 1) / u.rows_per_block);

  int status = ANIREC_OK;
  with_width(dim, [&](auto kd) {
    constexpr int kD = decltype(kd)::value;
    hipError_t e = hipFuncSetAttribute((const void *)k_kmeans_sums<kD>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kKmPartialBytes);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_kmeans_init, dim3(km_grid(n_rows)), dim3(kKmThreads), 0, s, S, ws_words, out_assign, n_rows);
      e = hipGetLastError();
    }
    for (int j = 1; j <= max_iter && e == hipSuccess; ++j) {
      a.changed = ctrl + 1 + j;
      u.changed = ctrl + 1 + j;
      e = km_launch_assign<kD>(a, s);
      if (e != hipSuccess) break;
      hipLaunchKernelGGL(k_kmeans_sums<kD>, dim3(sums_grid), dim3(kKmThreads), sums_lds, s, u);
      hipLaunchKernelGGL(k_kmeans_centroids, dim3((unsigned)((k + 63) / 64)), dim3(64), 0, s, C_inout,
                         reinterpret_cast<long long *>(S), k, dim, ctrl, ctrl + 1 + j, j);
      e = hipGetLastError();
    }
    if (e == hipSuccess) {
      a.changed = nullptr;  // max_iter iterations without a stop: the picks of the final centroids
      e = km_launch_assign<kD>(a, s);
    }
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_kmeans_tail, dim3((unsigned)((k + kKmThreads - 1) / kKmThreads)), dim3(kKmThreads), 0, s, ctrl,
                         max_iter, out_info, out_count, k);
      hipLaunchKernelGGL(k_kmeans_count, dim3(km_grid(n_rows)), dim3(kKmThreads), 0, s, out_assign, n_rows, k, out_count);
      e = hipGetLastError();
    }
    status = (int)e;
  });
  return status;
}

}  // extern "C"
