// Ranks to metric sums, and a Poisson bootstrap over users on those sums, for gfx950 (MI355X): include/anirec.h,
// anirec_rank_gain_rows / anirec_boot_sums / anirec_boot_weights.  Everything here is a sum of INTEGERS, so no result
// depends on how the work is dealt to lanes, waves or workgroups, or on the order the atomics land in.
//
// The statistic.  The resampling unit is the user: replicate b >= 1 gives unit u an integer weight w(b, u), independent
// over (b, u), drawn from a counter-based hash of (seed, b, the unit's KEY) and never stored; replicate 0 is the sample
// itself (all weights 1).  All arithmetic mod 2^32 on uint32:
//     mix32(x):      x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
//     r(seed,b,key)  = mix32( mix32(seed + 0x9e3779b9 * b)  ^  mix32(key + 0x85ebca6b) )
//     w              = #{ j < n_thr : r >= thr[j] }
// thr is the caller's ascending table of at most 16 entries (floor(2^32 CDF(j)) of Poisson(1) gives Poisson(1) weights,
// {0x80000000} half-sampling, an empty table all-zero weights).  The key is the unit's own number (the user index), not
// its position in the call, so a subset of the units gets the same weights in a call of its own.
//   gain rows  k_gain_rows: thread (chunk of kGainRun consecutive targets, column).  Consecutive lanes hold consecutive
//              columns of one chunk, so a wave's atomics land on contiguous int64 of a row; a thread adds up a run of
//              targets of one unit in a register and issues one atomic per run, so the targets of one unit, listed
//              together, cost 1 / kGainRun of their number in atomics.  Zero sums are not added.
//   boot sums  k_boot_partial: one lane is one replicate.  A 256-thread workgroup stages kBootTile units in LDS (the
//              pre-mixed key hash and the value rows of its column tile); every lane reads the same address (a
//              broadcast, no bank conflict), keeps its replicate's CT column sums in registers and pays per (replicate,
//              unit) one mix32, n_thr compares and CT widening multiply-adds.  grid = (replicate blocks, unit splits,
//              column tiles); a split takes every gridDim.y-th unit tile and stores its partial rows to the workspace.
//              k_boot_combine adds the partial rows in split order (int64: any order gives the same bits) and writes
//              -1 everywhere when a value broke the exactness guard.  No atomics; every workspace cell read was written
//              by the same call.
//   weights    k_boot_weights: thread per (replicate, unit), the same draw, one byte each.
#include <hip/hip_runtime.h>

#include "anirec_dev.hpp"

namespace anirec {

constexpr int kBootTile = 128;       // units staged per pass (anirec_boot_tile)
constexpr int kBootColNarrow = 8;    // column tile of a call with n_col <= 8
constexpr int kBootColWide = 24;     // column tile of a wider call: 24 int64 sums = 48 VGPRs
constexpr int kBootMaxCol = 4096;
constexpr int kBootMaxRep = 65536;
constexpr int kBootMaxThr = 16;
constexpr int kBootBlocks = 1024;    // workgroups a call aims for when it splits the units
constexpr int kGainRun = 16;         // consecutive targets one thread of k_gain_rows walks
constexpr int kGainMaxCol = 4096;

struct BootThr {
  uint32_t t[kBootMaxThr];
  int n;
};

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ uint32_t boot_rep_hash(uint32_t seed, uint32_t b) { return mix32(seed + 0x9e3779b9u * b); }
__device__ __forceinline__ uint32_t boot_key_hash(int32_t key) { return mix32((uint32_t)key + 0x85ebca6bu); }

// the weight of one (replicate hash, key hash) pair; thr lives in SGPRs, the test against n is the same in every lane
__device__ __forceinline__ uint32_t boot_weight(uint32_t hb, uint32_t hk, const BootThr &thr) {
  const uint32_t r = mix32(hb ^ hk);
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < kBootMaxThr; ++j)
    if (j < thr.n) w += r >= thr.t[j] ? 1u : 0u;
  return w;
}

template <int CT>
__global__ __launch_bounds__(256) void k_boot_partial(const long long *__restrict__ values,
                                                      const int32_t *__restrict__ unit_key, int n_units, int n_col,
                                                      uint32_t seed, int n_rep, BootThr thr, long long limit,
                                                      unsigned long long *__restrict__ part, int32_t *__restrict__ err) {
  __shared__ unsigned long long sv[kBootTile * CT];
  __shared__ uint32_t sk[kBootTile];
  const int tid = threadIdx.x;
  const int b = blockIdx.x * 256 + tid;   // the lane's replicate; lanes past n_rep compute and store nothing
  const int c0 = blockIdx.z * CT;
  const int nc = n_col - c0 < CT ? n_col - c0 : CT;
  const uint32_t hb = boot_rep_hash(seed, (uint32_t)b);
  unsigned long long acc[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) acc[c] = 0ull;
  const int n_tiles = (n_units + kBootTile - 1) / kBootTile;
  bool bad = false;
  for (int tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
    const int u0 = tile * kBootTile;
    const int cnt = n_units - u0 < kBootTile ? n_units - u0 : kBootTile;
    if (tid < kBootTile) sk[tid] = tid < cnt ? boot_key_hash(unit_key[u0 + tid]) : 0u;
    for (int i = tid; i < kBootTile * CT; i += 256) {
      const int u = i / CT, c = i % CT;
      long long v = 0;
      if (u < cnt && c < nc) {
        v = values[(size_t)(u0 + u) * (size_t)n_col + (size_t)(c0 + c)];
        bad = bad || v < 0 || v >= limit;
      }
      sv[i] = (unsigned long long)v;   // columns past n_col and units past the edge add zeros
    }
    __syncthreads();
    if (b == 0) {
      for (int u = 0; u < cnt; ++u) {
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] += sv[u * CT + c];
      }
    } else {
      for (int u = 0; u < cnt; ++u) {
        const uint32_t w = boot_weight(hb, sk[u], thr);
#pragma unroll
        for (int c = 0; c < CT; ++c) {  // w * v mod 2^64 from 32-bit halves: one widening multiply-add, one low multiply
          const unsigned long long v = sv[u * CT + c];
          acc[c] += (unsigned long long)w * (uint32_t)v + ((unsigned long long)(w * (uint32_t)(v >> 32)) << 32);
        }
      }
    }
    __syncthreads();
  }
  if (bad) *err = 1;
  if (b > n_rep) return;
  unsigned long long *row = part + ((size_t)blockIdx.y * (size_t)(n_rep + 1) + (size_t)b) * (size_t)n_col + (size_t)c0;
#pragma unroll
  for (int c = 0; c < CT; ++c)
    if (c < nc) row[c] = acc[c];
}

__global__ __launch_bounds__(256) void k_boot_combine(const unsigned long long *__restrict__ part, int n_splits,
                                                      size_t cells, const int32_t *__restrict__ err,
                                                      long long *__restrict__ out) {
  const bool bad = *err != 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += (size_t)gridDim.x * 256) {
    unsigned long long s = 0ull;
    for (int p = 0; p < n_splits; ++p) s += part[(size_t)p * cells + i];
    out[i] = bad ? -1ll : (long long)s;
  }
}

__global__ __launch_bounds__(256) void k_boot_weights(const int32_t *__restrict__ unit_key, int n_units, uint32_t seed,
                                                      int n_rep, BootThr thr, uint8_t *__restrict__ out) {
  const size_t total = (size_t)n_rep * (size_t)n_units;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const uint32_t b = (uint32_t)(i / (size_t)n_units) + 1u;
    const int u = (int)(i % (size_t)n_units);
    out[i] = (uint8_t)boot_weight(boot_rep_hash(seed, b), boot_key_hash(unit_key[u]), thr);
  }
}

__global__ __launch_bounds__(256) void k_gain_rows(const int32_t *__restrict__ ranks, int n_sys, int n_t,
                                                   const int32_t *__restrict__ target_unit, int n_units,
                                                   const uint32_t *__restrict__ gain, int n_metric, int n_gain,
                                                   unsigned long long *__restrict__ out, int32_t *__restrict__ err) {
  const int n_col = n_sys * n_metric + 1;
  const size_t n_chunk = ((size_t)n_t + kGainRun - 1) / kGainRun;
  const size_t total = n_chunk * (size_t)n_col;
  bool bad = false;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (size_t)gridDim.x * 256) {
    const int c = (int)(g % (size_t)n_col);
    const size_t t0 = g / (size_t)n_col * kGainRun;
    const int cnt = (size_t)n_t - t0 < (size_t)kGainRun ? (int)((size_t)n_t - t0) : kGainRun;
    const bool count_col = c == n_col - 1;
    const int32_t *rk = ranks + (count_col ? 0 : (size_t)(c / n_metric) * (size_t)n_t) + t0;
    const uint32_t *gm = gain + (count_col ? 0 : (size_t)(c % n_metric) * (size_t)n_gain);
    int cur = -1;
    unsigned long long run = 0ull;
    for (int i = 0; i < cnt; ++i) {
      const int u = target_unit[t0 + i];
      if ((uint32_t)u >= (uint32_t)n_units) {  // the target is dropped, nothing is addressed through it
        bad = true;
        continue;
      }
      if (u != cur) {
        if (run) atomicAdd(&out[(size_t)cur * (size_t)n_col + (size_t)c], run);
        cur = u;
        run = 0ull;
      }
      if (count_col) {
        run += 1ull;
      } else {
        const int r = rk[i];
        if ((uint32_t)r < (uint32_t)n_gain) run += (unsigned long long)gm[r];  // a rank outside the table gains 0
      }
    }
    if (run) atomicAdd(&out[(size_t)cur * (size_t)n_col + (size_t)c], run);
  }
  if (bad) *err = 1;
}

static int boot_col_tile(int32_t n_col) { return n_col <= kBootColNarrow ? kBootColNarrow : kBootColWide; }

// the unit splits of a call: enough workgroups to fill the chip, never more than there are unit tiles
static int boot_splits(int32_t n_units, int32_t n_col, int32_t n_rep) {
  const long long rep_blocks = ((long long)n_rep + 1 + 255) / 256;
  const int ct = boot_col_tile(n_col);
  const long long col_tiles = (n_col + ct - 1) / ct;
  const long long tiles = ((long long)n_units + kBootTile - 1) / kBootTile;
  long long s = (kBootBlocks + rep_blocks * col_tiles - 1) / (rep_blocks * col_tiles);
  if (s > tiles) s = tiles;
  if (s > 65535) s = 65535;
  return s < 1 ? 1 : (int)s;
}

static bool boot_thr_ok(const uint32_t *thr, int32_t n_thr) {
  if (n_thr < 0 || n_thr > kBootMaxThr || (n_thr > 0 && !thr)) return false;
  for (int j = 1; j < n_thr; ++j)
    if (thr[j] < thr[j - 1]) return false;
  return true;
}

static BootThr boot_thr(const uint32_t *thr, int32_t n_thr) {
  BootThr t;
  for (int j = 0; j < kBootMaxThr; ++j) t.t[j] = j < n_thr ? thr[j] : 0xFFFFFFFFu;
  t.n = n_thr;
  return t;
}

static unsigned grid_for(size_t total) {
  const size_t blocks = (total + 255) / 256;
  return (unsigned)(blocks < 1 ? 1 : blocks > 65536 ? 65536 : blocks);
}

}  // namespace anirec

using namespace anirec;

extern "C" {

size_t anirec_boot_tile(void) { return (size_t)kBootTile; }

size_t anirec_boot_col_tile(int32_t n_col) {
  if (n_col < 1 || n_col > kBootMaxCol) return 0;
  return (size_t)boot_col_tile(n_col);
}

size_t anirec_boot_workspace_bytes(int32_t n_units, int32_t n_col, int32_t n_rep) {
  if (n_units < 0 || n_col < 1 || n_col > kBootMaxCol || n_rep < 0 || n_rep > kBootMaxRep) return 0;
  if (n_units == 0) return 256;
  return (size_t)boot_splits(n_units, n_col, n_rep) * (size_t)(n_rep + 1) * (size_t)n_col * 8;
}

int anirec_boot_sums(const int64_t *values, const int32_t *unit_key, int32_t n_units, int32_t n_col, uint32_t seed,
                     int32_t n_rep, const uint32_t *thr, int32_t n_thr, int64_t *out, int32_t *err_flag, void *ws,
                     size_t ws_bytes, void *stream) {
  if (n_units < 0 || n_col < 1 || n_col > kBootMaxCol || n_rep < 0 || n_rep > kBootMaxRep || !boot_thr_ok(thr, n_thr))
    return ANIREC_EINVAL;
  if (!out || !err_flag || (n_units > 0 && (!values || !unit_key || !ws))) return ANIREC_EINVAL;
  if (((uintptr_t)out | (uintptr_t)values | (uintptr_t)ws) & 7) return ANIREC_EINVAL;
  if (n_units > 0 && ws_bytes < anirec_boot_workspace_bytes(n_units, n_col, n_rep)) return ANIREC_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  const size_t cells = (size_t)(n_rep + 1) * (size_t)n_col;
  if (n_units == 0) {
    ANIREC_HIP_CHECK(hipMemsetAsync(out, 0, cells * 8, s));
    return ANIREC_OK;
  }
  const long long limit = (1ll << 62) / ((long long)(n_thr > 1 ? n_thr : 1) * (long long)n_units);
  const BootThr t = boot_thr(thr, n_thr);
  const int ct = boot_col_tile(n_col), splits = boot_splits(n_units, n_col, n_rep);
  const dim3 grid(((unsigned)n_rep + 1u + 255u) / 256u, (unsigned)splits, (unsigned)((n_col + ct - 1) / ct));
  if (ct == kBootColNarrow)
    hipLaunchKernelGGL(k_boot_partial<kBootColNarrow>, grid, dim3(256), 0, s, (const long long *)values, unit_key,
                       n_units, n_col, seed, n_rep, t, limit, (unsigned long long *)ws, err_flag);
  else
    hipLaunchKernelGGL(k_boot_partial<kBootColWide>, grid, dim3(256), 0, s, (const long long *)values, unit_key, n_units,
                       n_col, seed, n_rep, t, limit, (unsigned long long *)ws, err_flag);
  hipLaunchKernelGGL(k_boot_combine, dim3(grid_for(cells)), dim3(256), 0, s, (const unsigned long long *)ws, splits,
                     cells, (const int32_t *)err_flag, (long long *)out);
  return (int)hipGetLastError();
}

int anirec_boot_weights(const int32_t *unit_key, int32_t n_units, uint32_t seed, int32_t n_rep, const uint32_t *thr,
                        int32_t n_thr, uint8_t *out, void *stream) {
  if (n_units < 0 || n_rep < 0 || n_rep > kBootMaxRep || !boot_thr_ok(thr, n_thr)) return ANIREC_EINVAL;
  if (n_units == 0 || n_rep == 0) return ANIREC_OK;
  if (!unit_key || !out) return ANIREC_EINVAL;
  const size_t total = (size_t)n_rep * (size_t)n_units;
  hipLaunchKernelGGL(k_boot_weights, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, unit_key, n_units, seed,
                     n_rep, boot_thr(thr, n_thr), out);
  return (int)hipGetLastError();
}

int anirec_rank_gain_rows(const int32_t *ranks, int32_t n_sys, int32_t n_t, const int32_t *target_unit, int32_t n_units,
                          const uint32_t *gain, int32_t n_metric, int32_t n_gain, int64_t *out, int32_t *err_flag,
                          void *stream) {
  if (n_sys < 1 || n_metric < 1 || n_gain < 1 || n_t < 0 || n_units < 0 ||
      (long long)n_sys * (long long)n_metric + 1 > kGainMaxCol)
    return ANIREC_EINVAL;
  if (!err_flag || (n_units > 0 && !out) || (n_t > 0 && (!ranks || !target_unit || !gain))) return ANIREC_EINVAL;
  if ((uintptr_t)out & 7) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const int n_col = n_sys * n_metric + 1;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  if (n_units > 0) ANIREC_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n_units * (size_t)n_col * 8, s));
  if (n_t == 0) return ANIREC_OK;
  const size_t total = (((size_t)n_t + kGainRun - 1) / kGainRun) * (size_t)n_col;
  hipLaunchKernelGGL(k_gain_rows, dim3(grid_for(total)), dim3(256), 0, s, ranks, n_sys, n_t, target_unit, n_units, gain,
                     n_metric, n_gain, (unsigned long long *)out, err_flag);
  return (int)hipGetLastError();
}

}  // extern "C"
