// Item-kNN from co-occurrence, for gfx950 (MI355X): include/anirec.h, anirec_cooc_scores / anirec_itemknn_scores.
// Everything here is a sum of INTEGERS (popcounts, fixed-point terms) followed by a fixed chain of correctly rounded
// fp64 operations, so no result depends on how the work is dealt to lanes, waves or workgroups, or on the order the
// atomics land in.
//   pop        k_cooc_pop: one wave per item row, lane l walks words l, l + 64, ...; the last word is masked with the
//              valid-bit word, the wave adds up once.  Written to the workspace (the epilogue's pop_q, pop_j) and, when
//              asked for, to out_pop.
//   counts     k_cooc: a 256-thread workgroup owns 64 queries x 64 keys.  Per pass it stages kCoocChunk = 64 user words
//              of both row sets in LDS (pitch 68 words: the 16 key rows of a ds_read_b128 fall on 16 distinct 16-byte
//              slots of the 256-byte bank row, the 4 query rows of a wave likewise), the last word of a row masked, rows
//              past the edge and rows of a bad query zero.  A thread keeps a 4 x 4 int32 block (queries ty + 16 r, keys
//              tx + 16 c); per four words it reads four uint4 of each set and runs 64 v_and + accumulating v_bcnt.
//   epilogue   counts -> sim / count / excl: den in fp64 (one rounding an operation, nothing contracted), one correctly
//              rounded divide, one rounding to fp32.  The excl words of a tile (two per query: a tile starts at a
//              multiple of 64 keys) are put together in LDS and stored whole, so the call writes every word once.
//   item-kNN   k_itemknn: one workgroup per list.  Entry e and slot s of its history x neighbour grid go to thread
//              (e * K + s) % 256; the term llrint(w * sim * 2^30) is added as int64, in LDS where n_items * 8 bytes fit
//              kKnnLdsBytes, else on the list's row of the workspace (zeroed by the call, read back past the L1).
#include <hip/hip_runtime.h>
#include <math.h>

#include "anirec_dev.hpp"

namespace anirec {

constexpr int kCoocTile = 64;    // queries and keys of one workgroup
constexpr int kCoocChunk = 64;   // user words staged per pass (anirec_cooc_chunk_words)
constexpr int kCoocPitch = 68;   // words between staged rows: 272 bytes, 16-byte aligned, 17 slots
constexpr size_t kKnnLdsBytes = 147456;  // 144 KiB of int64 sums: n_items <= 18432 accumulate in LDS
constexpr double kKnnScale = 1073741824.0;        // 2^30
constexpr double kKnnInvScale = 1.0 / 1073741824.0;
constexpr double kKnnMaxTerm = 1024.0;

struct CoocArgs {
  const uint32_t *bits;   // [n_items][W]
  int n_items, W;
  uint32_t last_mask;     // the valid bits of word W - 1
  const int32_t *queries; // [nq]
  int nq;
  int measure;
  double shrink;
  int minsup;             // max(1, min_support)
  float *out_sim;         // [nq][n_items]
  int32_t *out_count;     // optional [nq][n_items]
  uint32_t *out_excl;     // optional [nq][ewords]
  int ewords;
  const int32_t *pop;     // [n_items] (workspace)
  int32_t *err;
};

__global__ __launch_bounds__(256) void k_cooc_pop(const uint32_t *__restrict__ bits, int n_items, int W,
                                                  uint32_t last_mask, int32_t *__restrict__ pop,
                                                  int32_t *__restrict__ out_pop) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);  // the same for the whole wave
  if (i >= n_items) return;
  const uint32_t *row = bits + (size_t)i * W;
  int c = 0;
  for (int w = lane; w < W; w += 64) c += __popc(row[w] & (w == W - 1 ? last_mask : 0xFFFFFFFFu));
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) {
    pop[i] = c;
    if (out_pop) out_pop[i] = c;
  }
}

__device__ __forceinline__ float cooc_sim(int measure, int c, int pq, int pj, double shrink) {
#pragma clang fp contract(off)
  double den;
  if (measure == ANIREC_COOC_COSINE) {
    den = __dsqrt_rn((double)pq * (double)pj) + shrink;
  } else if (measure == ANIREC_COOC_JACCARD) {
    den = (double)((long long)pq + (long long)pj - (long long)c) + shrink;
  } else {
    den = (double)pq + shrink;
  }
  return (float)__ddiv_rn((double)c, den);
}

__global__ __launch_bounds__(256) void k_cooc(CoocArgs a) {
  __shared__ __align__(16) uint32_t sq[kCoocTile * kCoocPitch];
  __shared__ __align__(16) uint32_t sk[kCoocTile * kCoocPitch];
  __shared__ int qrow[kCoocTile];
  __shared__ uint32_t ex[kCoocTile][2];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int j0 = blockIdx.x * kCoocTile, q0 = blockIdx.y * kCoocTile;
  if (tid < kCoocTile) {
    const int t = q0 + tid;
    int q = -1;
    if (t < a.nq) {
      q = a.queries[t];
      if ((uint32_t)q >= (uint32_t)a.n_items) {  // nothing is read through a bad query
        q = -1;
        *a.err = 1;
      }
    }
    qrow[tid] = q;
    ex[tid][0] = 0u;
    ex[tid][1] = 0u;
  }
  __syncthreads();
  int acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0;

  for (int w0 = 0; w0 < a.W; w0 += kCoocChunk) {
#pragma unroll 4
    for (int i = tid; i < kCoocTile * kCoocChunk; i += 256) {
      const int r = i >> 6, w = i & 63, gw = w0 + w;
      uint32_t vq = 0u, vk = 0u;
      if (gw < a.W) {
        const uint32_t m = gw == a.W - 1 ? a.last_mask : 0xFFFFFFFFu;
        const int qr = qrow[r], j = j0 + r;
        if (qr >= 0) vq = a.bits[(size_t)qr * a.W + gw] & m;
        if (j < a.n_items) vk = a.bits[(size_t)j * a.W + gw] & m;
      }
      sq[r * kCoocPitch + w] = vq;
      sk[r * kCoocPitch + w] = vk;
    }
    __syncthreads();
    const int wl = a.W - w0 < kCoocChunk ? a.W - w0 : kCoocChunk;  // words past wl are staged zeros
    for (int w = 0; w < wl; w += 4) {
      uint4 qv[4], kv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) qv[r] = *(const uint4 *)&sq[(ty + 16 * r) * kCoocPitch + w];
#pragma unroll
      for (int c = 0; c < 4; ++c) kv[c] = *(const uint4 *)&sk[(tx + 16 * c) * kCoocPitch + w];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          acc[r][c] += __popc(qv[r].x & kv[c].x);
          acc[r][c] += __popc(qv[r].y & kv[c].y);
          acc[r][c] += __popc(qv[r].z & kv[c].z);
          acc[r][c] += __popc(qv[r].w & kv[c].w);
        }
    }
    __syncthreads();
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int lr = ty + 16 * r, t = q0 + lr;
    if (t >= a.nq) continue;
    const int qr = qrow[lr];
    const int pq = qr >= 0 ? a.pop[qr] : 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int lc = tx + 16 * c, j = j0 + lc;
      if (j >= a.n_items) continue;
      float sim;
      int cnt;
      bool excl;
      if (qr < 0) {
        sim = __uint_as_float(0x7FC00000u);
        cnt = -1;
        excl = true;
      } else {
        cnt = acc[r][c];
        const bool ok = cnt >= a.minsup;
        sim = ok ? cooc_sim(a.measure, cnt, pq, a.pop[j], a.shrink) : 0.0f;
        excl = !ok || j == qr;
      }
      const size_t o = (size_t)t * (size_t)a.n_items + (size_t)j;
      a.out_sim[o] = sim;
      if (a.out_count) a.out_count[o] = cnt;
      if (excl) atomicOr(&ex[lr][lc >> 5], 1u << (lc & 31));
    }
  }
  if (!a.out_excl) return;
  __syncthreads();
  if (tid < 2 * kCoocTile) {
    const int lr = tid >> 1, h = tid & 1, t = q0 + lr, wd = (j0 >> 5) + h;
    if (t < a.nq && wd < a.ewords) a.out_excl[(size_t)t * (size_t)a.ewords + wd] = ex[lr][h];
  }
}

struct KnnArgs {
  const int32_t *nbr_idx;  // [n_items][K]
  const float *nbr_sim;    // [n_items][K]
  int n_items, K;
  const int32_t *offsets;  // [n_lists + 1]
  const int32_t *hist_idx;
  const float *hist_w;     // optional
  int n_hist;
  float *out;              // [n_lists][n_items]
  unsigned long long *S;   // global form: [n_lists][n_items], zeroed by the call; LDS form: unused
  int32_t *err;
};

template <bool kLds>
__global__ __launch_bounds__(256) void k_itemknn(KnnArgs a) {
  extern __shared__ unsigned long long knn_sum[];
  const int tid = threadIdx.x;
  const size_t l = blockIdx.x;
  float *out = a.out + l * (size_t)a.n_items;
  const int lo = a.offsets[l], hi = a.offsets[l + 1];
  if (lo < 0 || hi < lo || hi > a.n_hist) {  // a bad pair: the row is NaN, nothing is read through it
    if (tid == 0) *a.err = 1;
    for (int j = tid; j < a.n_items; j += 256) out[j] = __uint_as_float(0x7FC00000u);
    return;
  }
  unsigned long long *S = kLds ? knn_sum : a.S + l * (size_t)a.n_items;
  if (kLds) {
    for (int j = tid; j < a.n_items; j += 256) S[j] = 0ull;
    __syncthreads();
  }
  const long long total = (long long)(hi - lo) * a.K;
  bool bad = false;
  for (long long p = tid; p < total; p += 256) {
    const int e = lo + (int)(p / a.K), s = (int)(p % a.K);
    const int i = a.hist_idx[e];
    if ((uint32_t)i >= (uint32_t)a.n_items) {
      bad = true;
      continue;
    }
    const int j = a.nbr_idx[(size_t)i * a.K + s];
    if (j < 0) continue;  // padding
    if (j >= a.n_items) {
      bad = true;
      continue;
    }
    const double w = a.hist_w ? (double)a.hist_w[e] : 1.0;
    const double prod = w * (double)a.nbr_sim[(size_t)i * a.K + s];  // exact: two 24-bit significands
    if (!(fabs(prod) <= kKnnMaxTerm)) {  // NaN, an infinite factor or a term past the documented range
      bad = true;
      continue;
    }
    const long long term = llrint(prod * kKnnScale);  // an exact scaling, rounded to the nearest even integer
    if (term) atomicAdd(&S[j], (unsigned long long)term);
  }
  if (bad) *a.err = 1;
  __syncthreads();
  for (int j = tid; j < a.n_items; j += 256) {
    const long long v = (long long)(kLds ? S[j] : __hip_atomic_load(&S[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    out[j] = (float)((double)v * kKnnInvScale);
  }
}

static size_t cooc_pop_bytes(int32_t n_items) { return ((size_t)n_items * 4 + 255) / 256 * 256; }
static bool knn_in_lds(int32_t n_items) { return (size_t)n_items * 8 <= kKnnLdsBytes; }

}  // namespace anirec

using namespace anirec;

extern "C" {

size_t anirec_cooc_chunk_words(void) { return (size_t)kCoocChunk; }

size_t anirec_cooc_workspace_bytes(int32_t n_items, int32_t nq) {
  if (n_items < 1 || nq < 0) return 0;
  return cooc_pop_bytes(n_items);
}

int anirec_cooc_scores(const uint32_t *item_bits, int32_t n_items, int32_t n_users, const int32_t *queries, int32_t nq,
                       int32_t measure, double shrink, int32_t min_support, float *out_sim, int32_t *out_count,
                       uint32_t *out_excl, int32_t *out_pop, int32_t *err_flag, void *ws, size_t ws_bytes,
                       void *stream) {
  if (n_items < 1 || n_users < 1 || nq < 0 || measure < ANIREC_COOC_COSINE || measure > ANIREC_COOC_CONFIDENCE ||
      !(shrink >= 0.0) || !(shrink <= 1.79769313486231570815e+308) || min_support < 0)
    return ANIREC_EINVAL;
  if (nq == 0) return ANIREC_OK;
  if (!item_bits || !queries || !out_sim || !err_flag || !ws) return ANIREC_EINVAL;
  if (ws_bytes < cooc_pop_bytes(n_items)) return ANIREC_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  CoocArgs a;
  a.bits = item_bits;
  a.n_items = n_items;
  a.W = (n_users + 31) / 32;
  a.last_mask = (n_users & 31) ? (1u << (n_users & 31)) - 1u : 0xFFFFFFFFu;
  a.queries = queries;
  a.nq = nq;
  a.measure = measure;
  a.shrink = shrink;
  a.minsup = min_support < 1 ? 1 : min_support;
  a.out_sim = out_sim;
  a.out_count = out_count;
  a.out_excl = out_excl;
  a.ewords = (n_items + 31) / 32;
  a.pop = (const int32_t *)ws;
  a.err = err_flag;
  hipLaunchKernelGGL(k_cooc_pop, dim3(((unsigned)n_items + 3u) / 4u), dim3(256), 0, s, item_bits, n_items, a.W,
                     a.last_mask, (int32_t *)ws, out_pop);
  const unsigned qt = ((unsigned)nq + kCoocTile - 1) / kCoocTile;
  const unsigned kt = ((unsigned)n_items + kCoocTile - 1) / kCoocTile;
  for (unsigned y0 = 0; y0 < qt; y0 += 32768u) {  // grid.y holds 65535 at the most
    CoocArgs b = a;
    const unsigned ny = qt - y0 < 32768u ? qt - y0 : 32768u;
    const size_t t0 = (size_t)y0 * kCoocTile;
    b.queries = a.queries + t0;
    b.nq = (int)((size_t)nq - t0 < (size_t)ny * kCoocTile ? (size_t)nq - t0 : (size_t)ny * kCoocTile);
    b.out_sim = a.out_sim + t0 * (size_t)n_items;
    if (a.out_count) b.out_count = a.out_count + t0 * (size_t)n_items;
    if (a.out_excl) b.out_excl = a.out_excl + t0 * (size_t)a.ewords;
    hipLaunchKernelGGL(k_cooc, dim3(kt, ny), dim3(256), 0, s, b);
  }
  return (int)hipGetLastError();
}

size_t anirec_itemknn_workspace_bytes(int32_t n_items, int32_t n_lists) {
  if (n_items < 1 || n_lists < 0) return 0;
  if (knn_in_lds(n_items) || n_lists == 0) return 256;
  return (size_t)n_lists * (size_t)n_items * 8;
}

size_t anirec_itemknn_lds_items(void) { return kKnnLdsBytes / 8; }

int anirec_itemknn_scores(const int32_t *nbr_idx, const float *nbr_sim, int32_t n_items, int32_t K,
                          const int32_t *hist_offsets, const int32_t *hist_idx, const float *hist_w, int32_t n_lists,
                          int32_t n_hist, float *out_scores, int32_t *err_flag, void *ws, size_t ws_bytes,
                          void *stream) {
  if (n_items < 1 || K < 1 || n_lists < 0 || n_hist < 0) return ANIREC_EINVAL;
  if (n_lists == 0) return ANIREC_OK;
  if (!nbr_idx || !nbr_sim || !hist_offsets || !out_scores || !err_flag || !ws || (n_hist > 0 && !hist_idx))
    return ANIREC_EINVAL;
  if (ws_bytes < anirec_itemknn_workspace_bytes(n_items, n_lists)) return ANIREC_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  KnnArgs a;
  a.nbr_idx = nbr_idx;
  a.nbr_sim = nbr_sim;
  a.n_items = n_items;
  a.K = K;
  a.offsets = hist_offsets;
  a.hist_idx = hist_idx;
  a.hist_w = hist_w;
  a.n_hist = n_hist;
  a.out = out_scores;
  a.S = (unsigned long long *)ws;
  a.err = err_flag;
  if (knn_in_lds(n_items)) {
    ANIREC_HIP_CHECK(hipFuncSetAttribute((const void *)k_itemknn<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)kKnnLdsBytes));
    hipLaunchKernelGGL(k_itemknn<true>, dim3(n_lists), dim3(256), (size_t)n_items * 8, s, a);
  } else {
    ANIREC_HIP_CHECK(hipMemsetAsync(ws, 0, (size_t)n_lists * (size_t)n_items * 8, s));
    hipLaunchKernelGGL(k_itemknn<false>, dim3(n_lists), dim3(256), 0, s, a);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
