// Onboarding lists by greedy maximum coverage, for gfx950 (MI355X): include/anirec.h, anirec_cover_greedy /
// anirec_cover_levels.  Every quantity is an integer count and the argmax key is a total order, so no result depends on
// how the rows are dealt to waves and workgroups or on the order the atomics land in.
//   init    k_cover_init: the open mask (open_bits or all ones, the last word cut to n_users), the candidate bytes
//           (keep), zeroed level planes, zeroed keys, the stop word.  The workspace needs no content on entry.
//   gain    k_cover_gain, once per pick: a wave per row, kCovWaves rows a workgroup at a time, a fixed grid walking the
//           rows.  The row is read as uint4 from its first 16-byte boundary (rows are only 4-byte aligned when W is odd:
//           up to 3 head and 3 tail words go one per lane), AND-ed with the open mask (LDS where it fits kCovLdsWords,
//           else global: it stays in L2) and popcounted; the mask's last word is already cut, so no word needs a
//           special case.  Rows that are no candidate are not read.  key = gain << 32 | 0xFFFFFFFF - index, the largest
//           per wave, then per workgroup through LDS, then ONE 64-bit atomicMax per workgroup on the pick's key word.
//   tail    k_cover_tail, once per pick, a thread per mask word: reads the key; gain 0 (no candidate leaves the key 0)
//           writes -1 / 0 and raises the stop word, on which every later gain launch returns at once (the later keys
//           stay 0, so the later tails pad too).  Else it writes the pick, clears its candidate byte and adds one to the
//           level of the row's open users: the levels are bit planes over the mask's words (ripple carry, word
//           parallel), a user whose level reaches depth leaves the open mask.  depth > m never closes anyone and keeps
//           no planes.
//   info    k_cover_info: one workgroup counts the keys with a gain, |P| and the users still open.
//   levels  k_cover_levels: a thread per user adds up its bit of the listed rows.
// No workgroup waits on another; every launch is a plain stream-ordered launch.
#include <hip/hip_runtime.h>

#include "anirec_dev.hpp"

namespace anirec {

constexpr int kCovThreads = 512;                  // a workgroup of the gain pass
constexpr int kCovWaves = kCovThreads / 64;       // rows it holds at a time: a wave per row
constexpr int kCovStep = 256;                     // words a wave covers per step of its row loop: 64 lanes x one uint4
constexpr int kCovMaxGroups = 768;                // the fixed grid of the gain pass: three workgroups a CU
constexpr int kCovLdsWords = 12288;               // the open mask is staged in LDS up to 48 KiB: 393 216 users
constexpr int kCovPlanes = 11;                    // level planes: levels 0 .. ANIREC_COVER_MAX_PICKS
constexpr size_t kCovCtrlBytes = 256;             // ctrl[0] = the stop word
constexpr size_t kCovKeyBytes = (size_t)ANIREC_COVER_MAX_PICKS * 8;

struct CoverLayout {
  size_t keys, open, planes, cand, total;
  size_t pitch;  // words between level planes
};

static CoverLayout cover_layout(int32_t n_items, int32_t n_users) {
  CoverLayout l;
  const size_t W = ((size_t)n_users + 31) / 32;
  l.pitch = (W + 63) / 64 * 64;
  l.keys = kCovCtrlBytes;
  l.open = l.keys + kCovKeyBytes;
  l.planes = l.open + l.pitch * 4;
  l.cand = l.planes + (size_t)kCovPlanes * l.pitch * 4;
  l.total = l.cand + ((size_t)n_items + 255) / 256 * 256;
  return l;
}

struct CoverInitArgs {
  const uint32_t *open_bits;  // optional [W]
  const uint8_t *keep;        // optional [n_items]
  int n_items, W, m;
  uint32_t last_mask;
  size_t plane_words;
  uint32_t *open, *planes;
  uint8_t *cand;
  unsigned long long *keys;
  int32_t *ctrl;
};

__global__ __launch_bounds__(256) void k_cover_init(CoverInitArgs a) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t < (size_t)a.W)
    a.open[t] = (a.open_bits ? a.open_bits[t] : 0xFFFFFFFFu) & (t == (size_t)a.W - 1 ? a.last_mask : 0xFFFFFFFFu);
  if (t < (size_t)a.n_items) a.cand[t] = a.keep ? (uint8_t)(a.keep[t] != 0) : (uint8_t)1;
  if (t < a.plane_words) a.planes[t] = 0u;
  if (t < (size_t)a.m) a.keys[t] = 0ull;
  if (t == 0) a.ctrl[0] = 0;
}

struct CoverGainArgs {
  const uint32_t *bits;  // [n_items][W]
  int n_items, W;
  const uint32_t *open;  // [W], the last word cut
  const uint8_t *cand;   // [n_items]
  const int32_t *done;
  unsigned long long *key;  // this pick's
};

// the wave's count of row & mask; every lane returns the sum
__device__ __forceinline__ int cover_row_gain(const uint32_t *__restrict__ row, const uint32_t *om, int W, int lane) {
  int head = (int)((4u - (uint32_t)(((uintptr_t)row >> 2) & 3u)) & 3u);  // words before the first 16-byte boundary
  if (head > W) head = W;
  int c = 0;
  if (lane < head) c += __popc(row[lane] & om[lane]);
  const int nvec = (W - head) >> 2;
  const uint4 *rv = (const uint4 *)(row + head);
  const uint32_t *ov = om + head;
#pragma unroll 4
  for (int v = lane; v < nvec; v += 64) {
    const uint4 r = rv[v];
    const uint32_t *o = ov + 4 * v;
    c += __popc(r.x & o[0]);
    c += __popc(r.y & o[1]);
    c += __popc(r.z & o[2]);
    c += __popc(r.w & o[3]);
  }
  const int t = head + 4 * nvec + lane;  // at most 3 words are left
  if (t < W) c += __popc(row[t] & om[t]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
  return c;
}

template <bool kLds>
__global__ __launch_bounds__(kCovThreads) void k_cover_gain(CoverGainArgs a) {
  extern __shared__ uint32_t cov_open[];
  __shared__ unsigned long long wbest[kCovWaves];
  if (*a.done) return;  // the same word for every thread of the launch
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (kLds) {
    for (int w = tid; w < a.W; w += kCovThreads) cov_open[w] = a.open[w];
    __syncthreads();
  }
  unsigned long long best = 0ull;
  const long long stride = (long long)gridDim.x * kCovWaves;
  for (long long i = (long long)blockIdx.x * kCovWaves + wave; i < a.n_items; i += stride) {
    if (!a.cand[i]) continue;  // the same for the whole wave
    const uint32_t *row = a.bits + (size_t)i * (size_t)a.W;
    const int c = kLds ? cover_row_gain(row, cov_open, a.W, lane) : cover_row_gain(row, a.open, a.W, lane);
    const unsigned long long key = ((unsigned long long)(uint32_t)c << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
    best = key > best ? key : best;
  }
  if (lane == 0) wbest[wave] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kCovWaves; ++w) best = wbest[w] > best ? wbest[w] : best;
    if (best) atomicMax(a.key, best);
  }
}

struct CoverTailArgs {
  const uint32_t *bits;
  int n_items, W;
  uint32_t *open, *planes;
  size_t pitch;
  int nb;      // level planes in use
  int depth;   // the level that closes a user; 0: nobody closes (depth > m)
  uint8_t *cand;
  int32_t *ctrl;
  const unsigned long long *key;
  int32_t *out_pick, *out_gain;  // this pick's
};

__global__ __launch_bounds__(256) void k_cover_tail(CoverTailArgs a) {
  const unsigned long long key = __hip_atomic_load(a.key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t gain = (uint32_t)(key >> 32);
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  const uint32_t i = 0xFFFFFFFFu - (uint32_t)key;
  if (gain == 0u || i >= (uint32_t)a.n_items) {  // no candidate, or nobody left to reach: the list ends here
    if (first) {
      *a.out_pick = -1;
      *a.out_gain = 0;
      a.ctrl[0] = 1;
    }
    return;
  }
  if (first) {
    *a.out_pick = (int32_t)i;
    *a.out_gain = (int32_t)gain;
    a.cand[i] = 0;
  }
  const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= (size_t)a.W) return;
  const uint32_t o = a.open[w];
  const uint32_t hit = a.bits[(size_t)i * (size_t)a.W + w] & o;
  if (!hit || a.nb == 0) return;
  uint32_t carry = hit, eq = hit;
  for (int k = 0; k < a.nb; ++k) {
    const uint32_t t = a.planes[(size_t)k * a.pitch + w];
    const uint32_t nv = t ^ carry;
    a.planes[(size_t)k * a.pitch + w] = nv;
    carry &= t;
    eq &= ((a.depth >> k) & 1) ? nv : ~nv;
  }
  if (a.depth) a.open[w] = o & ~eq;
}

__global__ __launch_bounds__(1024) void k_cover_info(const unsigned long long *keys, int m, const uint32_t *open_bits,
                                                     const uint32_t *open, int W, uint32_t last_mask,
                                                     int32_t *out_info) {
  __shared__ int s[3];
  const int tid = threadIdx.x;
  if (tid < 3) s[tid] = 0;
  __syncthreads();
  int made = 0, pn = 0, on = 0;
  for (int p = tid; p < m; p += 1024)
    made += (__hip_atomic_load(&keys[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32) != 0ull;
  for (int w = tid; w < W; w += 1024) {
    pn += __popc((open_bits ? open_bits[w] : 0xFFFFFFFFu) & (w == W - 1 ? last_mask : 0xFFFFFFFFu));
    on += __popc(open[w]);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    made += __shfl_xor(made, o, 64);
    pn += __shfl_xor(pn, o, 64);
    on += __shfl_xor(on, o, 64);
  }
  if ((tid & 63) == 0) {
    atomicAdd(&s[0], made);
    atomicAdd(&s[1], pn);
    atomicAdd(&s[2], on);
  }
  __syncthreads();
  if (tid == 0) {
    out_info[0] = s[0];
    out_info[1] = s[1] - s[2];
    out_info[2] = s[1];
    out_info[3] = 0;
  }
}

__global__ __launch_bounds__(256) void k_cover_levels(const uint32_t *__restrict__ bits, int n_items, int n_users, int W,
                                                      const int32_t *__restrict__ picks, int n_picks,
                                                      int32_t *__restrict__ out_level, int32_t *err) {
  const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= (size_t)n_users) return;
  const size_t w = u >> 5;
  const int b = (int)(u & 31);
  int c = 0;
  bool bad = false;
  for (int t = 0; t < n_picks; ++t) {
    const int i = picks[t];
    if (i == -1) continue;  // the padding of anirec_cover_greedy's out_pick
    if ((uint32_t)i >= (uint32_t)n_items) {  // nothing is read through a bad entry
      bad = true;
      continue;
    }
    c += (int)((bits[(size_t)i * (size_t)W + w] >> b) & 1u);
  }
  out_level[u] = c;
  if (bad && u == 0) *err = 1;
}

}  // namespace anirec

using namespace anirec;

extern "C" {

size_t anirec_cover_step_words(void) { return (size_t)kCovStep; }

size_t anirec_cover_lds_words(void) { return (size_t)kCovLdsWords; }

size_t anirec_cover_workspace_bytes(int32_t n_items, int32_t n_users) {
  if (n_items < 1 || n_users < 1) return 0;
  return cover_layout(n_items, n_users).total;
}

int anirec_cover_greedy(const uint32_t *item_bits, int32_t n_items, int32_t n_users, const uint32_t *open_bits,
                        const uint8_t *keep, int32_t depth, int32_t m, int32_t *out_pick, int32_t *out_gain,
                        int32_t *out_info, void *ws, size_t ws_bytes, void *stream) {
  if (n_items < 1 || n_users < 1 || depth < 1 || m < 1 || m > ANIREC_COVER_MAX_PICKS) return ANIREC_EINVAL;
  if (!item_bits || !out_pick || !out_gain || !out_info || !ws || ((uintptr_t)ws & 15)) return ANIREC_EINVAL;
  const CoverLayout l = cover_layout(n_items, n_users);
  if (ws_bytes < l.total) return ANIREC_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char *base = (char *)ws;
  int32_t *ctrl = (int32_t *)base;
  unsigned long long *keys = (unsigned long long *)(base + l.keys);
  uint32_t *open = (uint32_t *)(base + l.open);
  uint32_t *planes = (uint32_t *)(base + l.planes);
  uint8_t *cand = (uint8_t *)(base + l.cand);
  const int W = (int)(((int64_t)n_users + 31) / 32);
  const uint32_t last_mask = (n_users & 31) ? (1u << (n_users & 31)) - 1u : 0xFFFFFFFFu;
  const bool closes = depth <= m;
  int nb = 0;
  if (closes)
    for (int d = depth; d; d >>= 1) ++nb;  // levels 0 .. depth; nb <= kCovPlanes as depth <= m <= 1024

  CoverInitArgs ia;
  ia.open_bits = open_bits;
  ia.keep = keep;
  ia.n_items = n_items;
  ia.W = W;
  ia.m = m;
  ia.last_mask = last_mask;
  ia.plane_words = (size_t)nb * l.pitch;
  ia.open = open;
  ia.planes = planes;
  ia.cand = cand;
  ia.keys = keys;
  ia.ctrl = ctrl;
  size_t cells = (size_t)W;
  if ((size_t)n_items > cells) cells = (size_t)n_items;
  if (ia.plane_words > cells) cells = ia.plane_words;
  if ((size_t)m > cells) cells = (size_t)m;
  hipLaunchKernelGGL(k_cover_init, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, ia);

  CoverGainArgs ga;
  ga.bits = item_bits;
  ga.n_items = n_items;
  ga.W = W;
  ga.open = open;
  ga.cand = cand;
  ga.done = ctrl;
  CoverTailArgs ta;
  ta.bits = item_bits;
  ta.n_items = n_items;
  ta.W = W;
  ta.open = open;
  ta.planes = planes;
  ta.pitch = l.pitch;
  ta.nb = nb;
  ta.depth = closes ? depth : 0;
  ta.cand = cand;
  ta.ctrl = ctrl;
  const unsigned rows_groups = ((unsigned)n_items + kCovWaves - 1) / kCovWaves;
  const unsigned groups = rows_groups < (unsigned)kCovMaxGroups ? rows_groups : (unsigned)kCovMaxGroups;
  const unsigned tail_groups = ((unsigned)W + 255u) / 256u;
  const bool lds = W <= kCovLdsWords;
  for (int p = 0; p < m; ++p) {
    ga.key = keys + p;
    if (lds)
      hipLaunchKernelGGL(k_cover_gain<true>, dim3(groups), dim3(kCovThreads), (size_t)W * 4, s, ga);
    else
      hipLaunchKernelGGL(k_cover_gain<false>, dim3(groups), dim3(kCovThreads), 0, s, ga);
    ta.key = keys + p;
    ta.out_pick = out_pick + p;
    ta.out_gain = out_gain + p;
    hipLaunchKernelGGL(k_cover_tail, dim3(tail_groups), dim3(256), 0, s, ta);
  }
  hipLaunchKernelGGL(k_cover_info, dim3(1), dim3(1024), 0, s, keys, m, open_bits, open, W, last_mask, out_info);
  return (int)hipGetLastError();
}

int anirec_cover_levels(const uint32_t *item_bits, int32_t n_items, int32_t n_users, const int32_t *picks,
                        int32_t n_picks, int32_t *out_level, int32_t *err_flag, void *stream) {
  if (n_items < 1 || n_users < 1 || n_picks < 0) return ANIREC_EINVAL;
  if (!item_bits || !out_level || !err_flag || (n_picks > 0 && !picks)) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  const int W = (int)(((int64_t)n_users + 31) / 32);
  hipLaunchKernelGGL(k_cover_levels, dim3(((unsigned)n_users + 255u) / 256u), dim3(256), 0, s, item_bits, n_items, n_users,
                     W, picks, n_picks, out_level, err_flag);
  return (int)hipGetLastError();
}

}  // extern "C"
