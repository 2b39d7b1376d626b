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
// anirec_fuse_rank_grid (further down) ranks targets under many weight vectors at once from the same steps.
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

// ---- the rank grid (anirec_fuse_rank_grid) -----------------------------------------------------------
// The rank of every target under every weight vector, without a fused row.  What a term owes to the weights is one
// fp32 operation on a UNIT that does not depend on them: rrf_term(w, unit) with unit = c + 1 + r_s(t, j) as an int32,
// or w * unit with unit = minmax_term(1, x, lo, span) (1 * v is v).  Stage A writes the units once, stage B walks them.
//   ws        int32 / fp32 bits [n_rows][n_sys][npad], npad = n rounded up to kGridChunk; kGridNoUnit where an item is
//             not eligible and in the padding, so stage B needs neither the masks nor n's remainder
//   stage A   k_grid_units_rrf: k_fuse_rrf's image and sort per system, the thread that holds place r writes the unit;
//             k_grid_units_minmax: k_fuse_minmax's extrema, then one pass that writes v.  A workgroup per row.
//   stage B   k_grid_rank, a workgroup per (target, tile of 64 weight vectors): a lane is a weight vector and holds its
//             weights in registers; the waves split the row's chunks of four items, whose units are 16-byte loads at
//             one address for the whole wave; a lane forms each item's fused value in system order and counts the
//             order values above the target's own; the counts are added through LDS.  A tile that holds nv < 64
//             vectors (the last one) gives each vector 64 / 2^ceil(log2 nv) lanes, which split the chunks further, so
//             a grid of 67 costs little more than one of 64.  Integer counts: no result depends on the split.
constexpr int kGridChunk = 4;                  // items per 16-byte load of one system's units
constexpr int kGridTile = 64;                  // the most weight vectors of a workgroup: one per lane of a wave
constexpr int kGridWaves = 4;                  // waves of a stage B workgroup
constexpr uint32_t kGridNoUnit = 0xFFFFFFFFu;  // no unit: int32 -1 under rrf (a unit is >= 1), no value of v under minmax

struct GridArgs {
  FuseArgs f;            // rows, ld, n_sys, n, watched, wwords, keep, rrf_c; w, out and ld_out are not used
  uint32_t *units;       // [n_rows][n_sys][npad]
  int npad, n_rows;
  const float *weights;  // [n_w][n_sys]
  int n_w;
  const int32_t *target_row, *target_anime;
  int n_targets;
  int32_t *out_rank;     // [n_w][n_targets]
  int32_t *err;
};

__global__ __launch_bounds__(1024) void k_grid_units_rrf(GridArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long fuse_sw[];
  const FuseArgs &a = g.f;
  const int t = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int n = a.n;
  const uint32_t *wrow = a.watched ? a.watched + (size_t)t * a.wwords : nullptr;
  for (int s = 0; s < a.n_sys; ++s) {
    const float *row = a.rows[s] + (size_t)t * (size_t)a.ld[s];
    uint32_t *u = g.units + ((size_t)t * a.n_sys + s) * (size_t)g.npad;
    for (int j = tid; j < g.npad; j += nt) {
      const bool e = j < n && fuse_eligible(a, wrow, j);
      if (j < n)
        fuse_sw[j] = e ? ((unsigned long long)score_key(row[j]) << 32) | (unsigned long long)(~(uint32_t)j) : 0ull;
      if (!e) u[j] = kGridNoUnit;  // an eligible item's unit comes from the thread that holds its place
    }
    __syncthreads();
    lds_sort_desc(fuse_sw, (uint32_t)n, tid, nt);
    for (int r = tid; r < n; r += nt) {
      const unsigned long long v = fuse_sw[r];
      if (v == 0ull) continue;
      u[~(uint32_t)(v & 0xFFFFFFFFull)] = (uint32_t)(a.rrf_c + 1 + r);
    }
    __syncthreads();  // the image read before the next system loads it
  }
}

__global__ __launch_bounds__(1024) void k_grid_units_minmax(GridArgs g) {
  __shared__ uint32_t wmax[16], wmin[16];
  __shared__ float s_lo, s_span;
  const FuseArgs &a = g.f;
  const int t = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int n = a.n, nw = nt >> 6;
  const uint32_t *wrow = a.watched ? a.watched + (size_t)t * a.wwords : nullptr;
  for (int s = 0; s < a.n_sys; ++s) {
    const float *row = a.rows[s] + (size_t)t * (size_t)a.ld[s];
    uint32_t *u = g.units + ((size_t)t * a.n_sys + s) * (size_t)g.npad;
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
      if (mx != 0u) {
        const float hi = __uint_as_float((mx & 0x80000000u) ? (mx ^ 0x80000000u) : ~mx);
        lo = __uint_as_float((mn & 0x80000000u) ? (mn ^ 0x80000000u) : ~mn);
        span = hi - lo;
      }
      s_lo = lo;
      s_span = span;
    }
    __syncthreads();
    const float lo = s_lo, span = s_span;
    for (int j = tid; j < g.npad; j += nt) {
      const bool e = j < n && fuse_eligible(a, wrow, j);
      u[j] = e ? __float_as_uint(minmax_term(1.f, row[j], lo, span)) : kGridNoUnit;
    }
    __syncthreads();  // s_lo / s_span read before the next system writes them
  }
}

// one term of the fused value from a unit: the fp32 step of k_fuse_rrf / k_fuse_minmax that holds the weight
template <int METHOD>
__device__ __forceinline__ float grid_term(float w, uint32_t unit) {
#pragma clang fp contract(off)
  if (METHOD == ANIREC_FUSE_RRF) return rrf_term(w, (int)unit);
  return w * __uint_as_float(unit);
}

template <int METHOD>
__global__ __launch_bounds__(kGridTile *kGridWaves) void k_grid_rank(GridArgs g) {
  __shared__ int s_cnt[kGridWaves][kGridTile];
  const int S = g.f.n_sys, npad = g.npad;
  const int t = blockIdx.x, lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // the tile's nv vectors take P = 2^lgp >= nv lanes; the 64 / P lane groups of a wave each walk chunks of their own
  const int nv = min(kGridTile, g.n_w - (int)blockIdx.y * kGridTile);
  int lgp = 0;
  while ((1 << lgp) < nv) ++lgp;
  const int P = 1 << lgp, Q = kGridTile >> lgp;
  const int v = lane & (P - 1), q = lane >> lgp;
  const int wi = blockIdx.y * kGridTile + v;
  const bool live = v < nv;
  float w[ANIREC_FUSE_MAX_SYS];
  bool wok = true, wany = false;
#pragma unroll
  for (int s = 0; s < ANIREC_FUSE_MAX_SYS; ++s) {
    w[s] = (live && s < S) ? g.weights[(size_t)wi * S + s] : 0.f;
    wok = wok && w[s] >= 0.f && w[s] <= 3.402823466e+38f;  // negative, NaN or infinite
    wany = wany || w[s] > 0.f;
  }
  wok = wok && wany;
  const bool writer = wv == 0 && q == 0 && live;  // the one lane that stores the vector's rank of this target
  const int tr = g.target_row[t], ta = g.target_anime[t];
  bool tok = tr >= 0 && tr < g.n_rows && ta >= 0 && ta < g.f.n;
  const uint32_t *u = g.units + (size_t)(tok ? tr : 0) * S * (size_t)npad;
  tok = tok && u[ta] != kGridNoUnit;  // eligibility is the row's: every system holds the mark or none does
  if (!tok || !wok) {  // tok is the workgroup's, wok the vector's
    if (writer) {
      g.out_rank[(size_t)wi * g.n_targets + t] = -1;
      *g.err = 1;
    }
    if (!tok) return;
  }
  float ft = 0.f;
#pragma unroll
  for (int s = 0; s < ANIREC_FUSE_MAX_SYS; ++s)
    if (s < S) ft = fuse_add(ft, grid_term<METHOD>(w[s], u[(size_t)s * npad + ta]));
  const uint32_t kt = score_key(ft);
  int cnt = 0;
  for (int jb = (wv * Q + q) * kGridChunk; jb < npad; jb += kGridWaves * Q * kGridChunk) {
    uint4 c[ANIREC_FUSE_MAX_SYS];
#pragma unroll
    for (int s = 0; s < ANIREC_FUSE_MAX_SYS; ++s)
      if (s < S) c[s] = *(const uint4 *)(u + (size_t)s * npad + jb);
#pragma unroll
    for (int i = 0; i < kGridChunk; ++i) {
      const uint32_t u0 = i == 0 ? c[0].x : i == 1 ? c[0].y : i == 2 ? c[0].z : c[0].w;
      if (u0 == kGridNoUnit) continue;  // the same for the whole wave when the tile is full
      float f = 0.f;
#pragma unroll
      for (int s = 0; s < ANIREC_FUSE_MAX_SYS; ++s)
        if (s < S) {
          const uint32_t us = i == 0 ? c[s].x : i == 1 ? c[s].y : i == 2 ? c[s].z : c[s].w;
          f = fuse_add(f, grid_term<METHOD>(w[s], us));
        }
      const uint32_t kj = score_key(f);
      cnt += (kj > kt || (kj == kt && jb + i < ta)) ? 1 : 0;
    }
  }
  s_cnt[wv][lane] = cnt;
  __syncthreads();
  if (writer && wok) {
    int sum = 0;
    for (int k = 0; k < kGridWaves; ++k)
      for (int qq = 0; qq < Q; ++qq) sum += s_cnt[k][(qq << lgp) + v];
    g.out_rank[(size_t)wi * g.n_targets + t] = sum;
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

static size_t grid_npad(int32_t n) { return ((size_t)n + kGridChunk - 1) / kGridChunk * kGridChunk; }

size_t anirec_fuse_rank_grid_workspace_bytes(int32_t n_sys, int32_t n, int32_t n_rows, int32_t method) {
  if (n_sys < 1 || n_sys > ANIREC_FUSE_MAX_SYS || n < 1 || n > kLdsSortMax || n_rows < 0) return 0;
  if (method != ANIREC_FUSE_RRF && method != ANIREC_FUSE_MINMAX) return 0;
  return (size_t)n_rows * (size_t)n_sys * grid_npad(n) * sizeof(uint32_t);
}

int anirec_fuse_rank_grid(const float *const *rows_host, const int64_t *ld_host, int32_t n_sys, int32_t n,
                          int32_t n_rows, const uint32_t *watched, const uint8_t *keep, int32_t method, int32_t rrf_c,
                          const float *weights, int32_t n_w, const int32_t *target_row, const int32_t *target_anime,
                          int32_t n_targets, int32_t *out_rank, int32_t *err_flag, void *ws, size_t ws_bytes,
                          void *stream) {
  if (n_sys < 1 || n_sys > ANIREC_FUSE_MAX_SYS || n < 1 || n > kLdsSortMax || n_rows < 0) return ANIREC_EINVAL;
  if (method != ANIREC_FUSE_RRF && method != ANIREC_FUSE_MINMAX) return ANIREC_EINVAL;
  if (rrf_c < 0 || rrf_c > (1 << 20)) return ANIREC_EINVAL;
  if (n_w < 1 || n_w > ANIREC_FUSE_MAX_GRID || n_targets < 0) return ANIREC_EINVAL;
  if (!rows_host || !ld_host || !weights || !out_rank || !err_flag) return ANIREC_EINVAL;
  if (n_targets > 0 && (!target_row || !target_anime)) return ANIREC_EINVAL;
  GridArgs g;
  for (int s = 0; s < ANIREC_FUSE_MAX_SYS; ++s) {
    const bool used = s < n_sys;
    if (used && (!rows_host[s] || (ld_host[s] != 0 && ld_host[s] < (int64_t)n))) return ANIREC_EINVAL;
    g.f.rows[s] = used ? rows_host[s] : nullptr;
    g.f.ld[s] = used ? (long long)ld_host[s] : 0ll;
    g.f.w[s] = 0.f;
  }
  if (n_targets == 0 || n_rows == 0) return ANIREC_OK;
  if (ws_bytes < anirec_fuse_rank_grid_workspace_bytes(n_sys, n, n_rows, method)) return ANIREC_EWORKSPACE;
  if (!ws || ((uintptr_t)ws & 15u)) return ANIREC_EINVAL;
  g.f.n_sys = n_sys;
  g.f.n = n;
  g.f.watched = watched;
  g.f.wwords = (n + 31) / 32;
  g.f.keep = keep;
  g.f.rrf_c = rrf_c;
  g.f.out = nullptr;
  g.f.ld_out = 0;
  g.units = (uint32_t *)ws;
  g.npad = (int)grid_npad(n);
  g.n_rows = n_rows;
  g.weights = weights;
  g.n_w = n_w;
  g.target_row = target_row;
  g.target_anime = target_anime;
  g.n_targets = n_targets;
  g.out_rank = out_rank;
  g.err = err_flag;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  const dim3 grid_b((unsigned)n_targets, (unsigned)((n_w + kGridTile - 1) / kGridTile));
  if (method == ANIREC_FUSE_MINMAX) {
    const int nt = n >= 1024 ? 1024 : (n + 63) / 64 * 64;
    hipLaunchKernelGGL(k_grid_units_minmax, dim3(n_rows), dim3(nt), 0, s, g);
    hipLaunchKernelGGL(k_grid_rank<ANIREC_FUSE_MINMAX>, grid_b, dim3(kGridTile * kGridWaves), 0, s, g);
    return (int)hipGetLastError();
  }
  ANIREC_HIP_CHECK(hipFuncSetAttribute((const void *)k_grid_units_rrf, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kLdsSortMax * 8));
  uint32_t p2 = 1;
  while (p2 < (uint32_t)n) p2 <<= 1;
  const int nt = p2 / 2 < 64 ? 64 : (p2 / 2 > 1024 ? 1024 : (int)(p2 / 2));
  hipLaunchKernelGGL(k_grid_units_rrf, dim3(n_rows), dim3(nt), (size_t)n * 8, s, g);
  hipLaunchKernelGGL(k_grid_rank<ANIREC_FUSE_RRF>, grid_b, dim3(kGridTile * kGridWaves), 0, s, g);
  return (int)hipGetLastError();
}

}  // extern "C"
