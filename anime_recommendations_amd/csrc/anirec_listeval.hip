// Pairwise similarity structure of many lists for gfx950 (MI355X): include/anirec.h, anirec_list_similarity.  A list
// of k slots (rows of the normalised table What, -1 = empty) gets, per present slot s, the sequential fp32 sum and the
// running maximum of sim(s, j) over the present slots j before it.  The lists share nothing but the table, so a call is
//   k_listsim  a GROUP of kG lanes per list; a workgroup holds kLists = blockDim / kG lists, each with its own LDS slice.
//     check    every index of the list is validated before anything is read through one (a bad one: the list's
//              outputs become NaN, *err = 1, nothing gathered) — k_mmr's check.
//     stage    the list's rows are gathered ONCE into LDS as float4 columns: img[v][c] = What[idx_c][4v .. 4v + 3], row
//              pitch P = k | 1 float4.  A wave reads 8 rows x 128 B per instruction (whole cache lines); its
//              ds_write_b128 is conflict-free: a group of 8 lanes holds 8 consecutive v of one slot, the 16-byte bank
//              slots (v P + c) mod 8 are all distinct for odd P.
//     pairs    the work is a triangle (slot s has s partners), so the lanes do not own slots: the pairs (s, j < s) of a
//              block of rows are numbered along the triangle and dealt round the group, every lane the same count to
//              within one.  A pair is one k-ordered fma chain down the image.  A wave's lane takes one pair at a time:
//              two ds_read_b128 per four fmas; lanes of consecutive j read consecutive 16-byte slots, lanes of one s
//              the same address (a broadcast).  A workgroup's lane takes a 2 x 2 tile of pairs, slots (2a, 2a + 1) x
//              (2b, 2b + 1): four chains share four reads, half the LDS traffic per fma (the tiles of the diagonal hold
//              one pair).  Each chain is the same sequence of fmas either way.  Results go to sim[s - r0][j] (row
//              pitch k | 1 floats).
//     fold     lane i of the group walks row r0 + i of sim over the present j in ascending order: sum = sum + sim, and
//              max by mmr's pen rule, as selects, so that the reads run ahead of the adds.  The odd pitch keeps the
//              lanes on distinct banks.  Rows come in blocks of R = min(k, kSimFloats / (k | 1)) (even when there is
//              more than one) so that the k x k matrix is never formed: one block while k <= 64.
// Group size: a list of 10 slots is 45 chains and 5.6 KiB at width 128 — a workgroup per list would leave three waves
// in four idle — so a list gets one wave (kG = 64, four lists a workgroup) while k <= 32 and four lists' slices fit
// 64 KiB, and a whole workgroup (kG = 256) beyond.  No workspace, no atomics; err is a plain store of the one value 1.
#include <hip/hip_runtime.h>
#include <math.h>

#include "anirec_dev.hpp"

namespace anirec {

constexpr int kLsThreads = 256;
constexpr int kLsImageFloats = 32768;   // dim * k at most: anirec_mmr_max_cand's row image
constexpr int kLsSimFloats = 64 * 65;   // a block of sim rows; a list of up to 64 slots is one block
constexpr int kLsWaveK = 32;            // the longest list a single wave takes
constexpr size_t kLsWaveBytes = 65536;  // ... while four such lists fit this much LDS

struct ListSimArgs {
  const float *What;        // [n_rows][dim] unit rows
  int n_rows;
  const int32_t *list_idx;  // [n_lists][k], -1 = empty slot
  int n_lists, k;
  int rows_per_block;       // R
  int slice_floats;         // LDS floats of one list's slice (a multiple of 4)
  float *out_max, *out_sum; // [n_lists][k]
  int32_t *err;
};

// host and device: the rows of sim a block holds, and the LDS floats of one list
static inline __host__ __device__ int ls_rows_per_block(int k) {
  const int r = kLsSimFloats / (k | 1);
  return r < k ? (r & ~1) : k;  // (even, so that a later block starts on a pair of rows)
}
static inline __host__ __device__ int ls_slice_floats(int dim, int k) {
  const int f = dim * (k | 1) + ls_rows_per_block(k) * (k | 1) + k;
  return (f + 3) & ~3;
}

// OR of a flag over the group: a wave (kG == 64) or the whole workgroup
template <int kG>
__device__ __forceinline__ int group_or(int v) {
  if constexpr (kG == 64) {
    return __any(v);
  } else {
    return __syncthreads_or(v);
  }
}

// ((sum + sim)): a plain rounded add
__device__ __forceinline__ float ls_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

template <int kD, int kG>
__global__ __launch_bounds__(kLsThreads) void k_listsim(ListSimArgs a) {
  constexpr int kRowV = kD / 4;  // float4 per row
  extern __shared__ __attribute__((aligned(16))) float ls_smem[];
  const int g = threadIdx.x % kG, k = a.k;
  const int P = k | 1;
  const long long l = (long long)blockIdx.x * (blockDim.x / kG) + threadIdx.x / kG;
  const bool active = l < a.n_lists;
  float *slice = ls_smem + (size_t)(threadIdx.x / kG) * a.slice_floats;
  float4 *img = reinterpret_cast<float4 *>(slice);                 // [kRowV][P]
  float *sim = slice + (size_t)kD * P;                             // [R][P]
  int32_t *row_of = reinterpret_cast<int32_t *>(sim + (size_t)a.rows_per_block * P);  // [k] table row, -1 = empty
  const int32_t *lidx = a.list_idx + (active ? l : 0) * (long long)k;
  float *o_max = a.out_max + (active ? l : 0) * (long long)k, *o_sum = a.out_sum + (active ? l : 0) * (long long)k;
  const float nanv = __uint_as_float(0x7FC00000u);

  // check: nothing is read through an index before every index of the list has passed
  int bad = 0;
  if (active) {
    for (int c = g; c < k; c += kG) {
      const int32_t r = lidx[c];
      bad |= (r < -1 || r >= a.n_rows);
      row_of[c] = r;
    }
  }
  bad = group_or<kG>(bad);
  const bool work = active && !bad;
  if (active && bad) {
    if (g == 0) *a.err = 1;
    for (int s = g; s < k; s += kG) {
      o_max[s] = nanv;
      o_sum[s] = nanv;
    }
  }
  __syncthreads();

  // stage: unit e = 8 float4 columns (e & 7) of one slot; 8 consecutive slots per wave instruction
  if (work) {
    for (int e = g; e < k * kRowV; e += kG) {
      const int q = e >> 3;
      const int c = q % k, v = (q / k) * 8 + (e & 7);
      const int32_t r = row_of[c];
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r >= 0) x = reinterpret_cast<const float4 *>(a.What)[(size_t)r * kRowV + v];
      img[v * P + c] = x;
    }
  }
  __syncthreads();

  for (int r0 = 0; r0 < k; r0 += a.rows_per_block) {
    const int r1 = min(k, r0 + a.rows_per_block);
    if (work) {
      if constexpr (kG == 64) {
        // pairs: q numbers the pairs along the triangle, row s holds q in [s (s - 1) / 2, s (s + 1) / 2)
        const int base = r0 * (r0 - 1) / 2, end = r1 * (r1 - 1) / 2;
        for (int q = base + g; q < end; q += kG) {
          int s = (int)((1.f + sqrtf(1.f + 8.f * (float)q)) * 0.5f);
          while (s * (s - 1) / 2 > q) --s;
          while (s * (s + 1) / 2 <= q) ++s;
          const int j = q - s * (s - 1) / 2;
          const float4 *ps = img + s, *pj = img + j;
          float acc = 0.f;
#pragma unroll 8
          for (int v = 0; v < kRowV; ++v) {
            const float4 x = ps[v * P], y = pj[v * P];
            acc = __fmaf_rn(x.x, y.x, acc);
            acc = __fmaf_rn(x.y, y.y, acc);
            acc = __fmaf_rn(x.z, y.z, acc);
            acc = __fmaf_rn(x.w, y.w, acc);
          }
          sim[(s - r0) * P + j] = acc;
        }
      } else {
        // tiles: slots (2a, 2a + 1) x (2b, 2b + 1), b <= a, numbered along the triangle of tiles (row a holds q in
        // [a (a + 1) / 2, (a + 1) (a + 2) / 2)): four chains share four reads.  r0 is even; a tile on the diagonal
        // holds the one pair (2a + 1, 2a), and slot k of an odd k is read as slot k - 1 and not written.
        const int a0 = r0 / 2, a1 = (r1 + 1) / 2;
        const int base = a0 * (a0 + 1) / 2, end = a1 * (a1 + 1) / 2;
        for (int q = base + g; q < end; q += kG) {
          int ta = (int)((sqrtf(1.f + 8.f * (float)q) - 1.f) * 0.5f);
          while (ta * (ta + 1) / 2 > q) --ta;
          while ((ta + 1) * (ta + 2) / 2 <= q) ++ta;
          const int tb = q - ta * (ta + 1) / 2;
          const int s0 = 2 * ta, s1 = min(s0 + 1, k - 1), j0 = 2 * tb, j1 = min(j0 + 1, k - 1);
          const float4 *p0 = img + s0, *p1 = img + s1, *q0 = img + j0, *q1 = img + j1;
          float c00 = 0.f, c01 = 0.f, c10 = 0.f, c11 = 0.f;
#pragma unroll 4
          for (int v = 0; v < kRowV; ++v) {
            const float4 x0 = p0[v * P], x1 = p1[v * P], y0 = q0[v * P], y1 = q1[v * P];
            c00 = __fmaf_rn(x0.x, y0.x, c00);
            c01 = __fmaf_rn(x0.x, y1.x, c01);
            c10 = __fmaf_rn(x1.x, y0.x, c10);
            c11 = __fmaf_rn(x1.x, y1.x, c11);
            c00 = __fmaf_rn(x0.y, y0.y, c00);
            c01 = __fmaf_rn(x0.y, y1.y, c01);
            c10 = __fmaf_rn(x1.y, y0.y, c10);
            c11 = __fmaf_rn(x1.y, y1.y, c11);
            c00 = __fmaf_rn(x0.z, y0.z, c00);
            c01 = __fmaf_rn(x0.z, y1.z, c01);
            c10 = __fmaf_rn(x1.z, y0.z, c10);
            c11 = __fmaf_rn(x1.z, y1.z, c11);
            c00 = __fmaf_rn(x0.w, y0.w, c00);
            c01 = __fmaf_rn(x0.w, y1.w, c01);
            c10 = __fmaf_rn(x1.w, y0.w, c10);
            c11 = __fmaf_rn(x1.w, y1.w, c11);
          }
          float *d0 = sim + (s0 - r0) * P + j0, *d1 = d0 + P;
          const bool below = tb < ta, odd = s0 + 1 < k;
          if (below) {
            d0[0] = c00;
            d0[1] = c01;
          }
          if (odd) d1[0] = c10;
          if (odd && below) d1[1] = c11;
        }
      }
    }
    __syncthreads();
    // fold: the present partners of slot s in ascending position
    if (work && r0 + g < r1) {
      const int s = r0 + g;
      float sum = nanv, mx = nanv;
      if (row_of[s] >= 0) {
        const float *srow = sim + g * P;
        sum = 0.f;
        mx = 0.f;
        bool first = true;
        // selects, not branches: the reads of the next partners do not wait for the chain of adds
#pragma unroll 8
        for (int j = 0; j < s; ++j) {
          const bool there = row_of[j] >= 0;
          const float x = srow[j];
          sum = there ? ls_add(sum, x) : sum;
          mx = (there && (first || x > mx)) ? x : mx;
          first = first && !there;
        }
      }
      o_max[s] = mx;
      o_sum[s] = sum;
    }
    __syncthreads();
  }
}

}  // namespace anirec

using namespace anirec;

extern "C" {

int anirec_list_similarity(const float *What, int32_t dim, int32_t n_rows, const int32_t *list_idx, int32_t n_lists,
                           int32_t k, float *out_sim_max, float *out_sim_sum, int32_t *err_flag, void *stream) {
  if (!dim_ok(dim) || n_rows < 1 || n_lists < 0 || k < 1 || k > kLsImageFloats / dim) return ANIREC_EINVAL;
  if (n_lists == 0) return ANIREC_OK;
  if (!What || !list_idx || !out_sim_max || !out_sim_sum || !err_flag) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ListSimArgs a;
  a.What = What;
  a.n_rows = n_rows;
  a.list_idx = list_idx;
  a.n_lists = n_lists;
  a.k = k;
  a.rows_per_block = ls_rows_per_block(k);
  a.slice_floats = ls_slice_floats(dim, k);
  a.out_max = out_sim_max;
  a.out_sum = out_sim_sum;
  a.err = err_flag;
  const size_t slice = (size_t)a.slice_floats * sizeof(float);
  const bool wave = k <= kLsWaveK && 4 * slice <= kLsWaveBytes;
  int status = ANIREC_OK;
  with_width(dim, [&](auto kd) {
    constexpr int kD = decltype(kd)::value;
    const auto launch = [&](auto kernel, int lists) {
      const size_t lds = slice * lists;
      hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e == hipSuccess) e = hipMemsetAsync(err_flag, 0, sizeof(int32_t), s);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)(((long long)n_lists + lists - 1) / lists)), dim3(kLsThreads), lds, s, a);
        e = hipGetLastError();
      }
      status = (int)e;
    };
    if (wave) {
      launch(k_listsim<kD, 64>, kLsThreads / 64);
    } else {
      launch(k_listsim<kD, kLsThreads>, 1);
    }
  });
  return status;
}

}  // extern "C"
