// Greedy maximal-marginal-relevance (MMR) re-rank of candidate lists for gfx950 (MI355X): include/anirec.h,
// anirec_mmr_rerank.  A list of n_cand candidates (rows of the normalised table What, with a relevance score each)
// becomes a list of k picks; each pick maximises  lambda * score - (1 - lambda) * (largest cosine to a row already
// picked).  The lists share nothing but the table, so a call is
//   k_mmr      one workgroup of 256 lanes per list, every pick inside the one launch.
//     check    every index of the list is validated before anything is read through one (a bad one: the list's
//              outputs become -1 / NaN, *err = 1, nothing gathered).
//     stage    the rows of the list's candidates are gathered ONCE into LDS, k-major: img[t][c] = What[idx_c][t] with
//              row pitch P = n_cand | 1.  A wave reads 8 rows x 128 B per instruction (whole cache lines) and its
//              transposed ds_write_b32 is conflict-free: a 32-lane half holds 8 float4 columns x 4 candidates, the
//              banks (4 v P + j P + c) mod 32 are all distinct for odd P.  A row with a non-finite element marks its
//              candidate absent.
//     pick     lane i owns candidates i, i + 256, ...: score, pen and the present/picked state live in registers.
//              val -> an order-preserving 32-bit key (NaN after every number, -0 == +0), packed over ~position, and a
//              workgroup max (wave butterfly, then 4 words through LDS; the two scratch rows alternate, so a pick
//              costs one barrier).  The owner of the winner writes the four outputs.
//     update   lane i walks the k-ordered fma chain of (candidate i, picked row) down the image: its own column is
//              a conflict-free ds_read_b32 stream, the picked column a broadcast.  n_cand chains a pick — the
//              n_cand x n_cand matrix is never formed.
// LDS: (dim * P + 2 * n_cand) floats, sized per launch: 51.3 KiB for 100 x 128 (three workgroups a CU), at most
// 136.1 KiB (1024 x 32) of the CU's 160 KiB.  No workspace, no atomics; err is a plain store of the one value 1.
#include <hip/hip_runtime.h>
#include <math.h>

#include "anirec_dev.hpp"

namespace anirec {

constexpr int kMmrThreads = 256;
constexpr int kMmrImageFloats = 32768;  // dim * n_cand at most: the 128 KiB row image

struct MmrArgs {
  const float *What;          // [n_rows][dim] unit rows
  int n_rows;
  const int32_t *cand_idx;    // [n_lists][n_cand], -1 = empty slot
  const float *cand_score;    // [n_lists][n_cand]
  int n_cand, k;
  float lambda, oml;          // oml = 1.0f - lambda
  int32_t *out_idx, *out_pos; // [n_lists][k]
  float *out_score, *out_pen; // [n_lists][k]
  int32_t *err;
};

template <int kD>
__global__ __launch_bounds__(kMmrThreads) void k_mmr(MmrArgs a) {
  constexpr int kRowV = kD / 4;                                              // float4 per row
  constexpr int kSlots = (kMmrImageFloats / kD + kMmrThreads - 1) / kMmrThreads;  // candidates a lane owns: 4, 2, 1, 1
  extern __shared__ __attribute__((aligned(16))) float mmr_smem[];
  __shared__ unsigned long long best_w[2][kMmrThreads / 64];
  const int tid = threadIdx.x, n = a.n_cand, k = a.k;
  const int P = n | 1;
  float *img = mmr_smem;                                       // [kD][P]
  int32_t *row_of = reinterpret_cast<int32_t *>(img + (size_t)kD * P);  // [n] table row, -1 = empty
  int32_t *row_bad = row_of + n;                               // [n] 1 = a non-finite element
  const size_t l = blockIdx.x;
  const int32_t *cidx = a.cand_idx + l * (size_t)n;
  const float *cscore = a.cand_score + l * (size_t)n;
  int32_t *o_idx = a.out_idx + l * (size_t)k, *o_pos = a.out_pos + l * (size_t)k;
  float *o_score = a.out_score + l * (size_t)k, *o_pen = a.out_pen + l * (size_t)k;
  const float nanv = __uint_as_float(0x7FC00000u);

  // check: nothing is read through an index before every index of the list has passed
  int bad = 0;
  for (int c = tid; c < n; c += kMmrThreads) {
    const int32_t r = cidx[c];
    bad |= (r < -1 || r >= a.n_rows);
    row_of[c] = r;
    row_bad[c] = 0;
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) *a.err = 1;
    for (int s = tid; s < k; s += kMmrThreads) {
      o_idx[s] = -1;
      o_pos[s] = -1;
      o_score[s] = nanv;
      o_pen[s] = nanv;
    }
    return;
  }

  // stage: unit e = 8 float4 columns (e & 7) of one candidate; 8 consecutive candidates per wave instruction
  for (int e = tid; e < n * kRowV; e += kMmrThreads) {
    const int q = e >> 3;
    const int c = q % n, v = (q / n) * 8 + (e & 7);
    const int32_t r = row_of[c];
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r >= 0) {
      x = reinterpret_cast<const float4 *>(a.What)[(size_t)r * kRowV + v];
      const uint32_t inf = 0x7F800000u;
      if ((__float_as_uint(x.x) & inf) == inf || (__float_as_uint(x.y) & inf) == inf ||
          (__float_as_uint(x.z) & inf) == inf || (__float_as_uint(x.w) & inf) == inf)
        row_bad[c] = 1;
    }
    float *d = img + (size_t)(4 * v) * P + c;
    d[0] = x.x;
    d[P] = x.y;
    d[2 * P] = x.z;
    d[3 * P] = x.w;
  }
  __syncthreads();

  float sc[kSlots], ls[kSlots], pen[kSlots];
  bool live[kSlots];  // present and not yet picked
#pragma unroll
  for (int j = 0; j < kSlots; ++j) {
    const int c = tid + j * kMmrThreads;
    sc[j] = 0.f;
    live[j] = false;
    if (c < n) {
      sc[j] = cscore[c];
      live[j] = row_of[c] >= 0 && !(sc[j] != sc[j]) && !row_bad[c];
    }
    ls[j] = mmr_mul(a.lambda, sc[j]);
    pen[j] = 0.f;
  }

  int s = 0;
  for (; s < k; ++s) {
    unsigned long long mine = 0ull;
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      if (live[j]) {
        const uint32_t c = tid + j * kMmrThreads;
        const unsigned long long w = ((unsigned long long)mmr_key(mmr_val(ls[j], a.oml, pen[j])) << 32) | (0xFFFFFFFFu - c);
        mine = w > mine ? w : mine;
      }
    }
    mine = wave_max_u64(mine);
    if ((tid & 63) == 0) best_w[s & 1][tid >> 6] = mine;
    __syncthreads();
    unsigned long long best = best_w[s & 1][0];
#pragma unroll
    for (int w = 1; w < kMmrThreads / 64; ++w) best = best_w[s & 1][w] > best ? best_w[s & 1][w] : best;
    if ((best >> 32) == 0ull) break;  // no present candidate is left (uniform over the workgroup)
    const int pos = (int)(0xFFFFFFFFu - (uint32_t)best);
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      if (pos == tid + j * kMmrThreads) {
        o_idx[s] = row_of[pos];
        o_pos[s] = pos;
        o_score[s] = sc[j];
        o_pen[s] = pen[j];
        live[j] = false;
      }
    }
    if (s + 1 == k) continue;
    // update: sim(i, pos) by the k-ordered chain, for the candidates still in play
    const float *pp = img + pos;
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      if (!live[j]) continue;
      const float *pi = img + tid + j * kMmrThreads;
      float sim = 0.f;
#pragma unroll 8
      for (int t = 0; t < kD; ++t) sim = __fmaf_rn(pi[t * P], pp[t * P], sim);
      pen[j] = (s == 0 || sim > pen[j]) ? sim : pen[j];
    }
  }
  // fewer than k present candidates: the rest of the row
  for (int r = s + tid; r < k; r += kMmrThreads) {
    o_idx[r] = -1;
    o_pos[r] = -1;
    o_score[r] = nanv;
    o_pen[r] = nanv;
  }
}

}  // namespace anirec

using namespace anirec;

extern "C" {

size_t anirec_mmr_max_cand(int32_t dim) { return dim_ok(dim) ? (size_t)(kMmrImageFloats / dim) : 0; }

int anirec_mmr_rerank(const float *What, int32_t dim, int32_t n_rows, const int32_t *cand_idx, const float *cand_score,
                      int32_t n_lists, int32_t n_cand, int32_t k, float lambda, int32_t *out_idx, int32_t *out_pos,
                      float *out_score, float *out_pen, int32_t *err_flag, void *stream) {
  if (!dim_ok(dim) || n_rows < 1 || n_lists < 0 || n_cand < 0 || k < 1 || k > n_cand ||
      (size_t)n_cand > anirec_mmr_max_cand(dim) || !(lambda >= 0.f && lambda <= 1.f))
    return ANIREC_EINVAL;
  if (n_lists == 0) return ANIREC_OK;
  if (!What || !cand_idx || !cand_score || !out_idx || !out_pos || !out_score || !out_pen || !err_flag)
    return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  MmrArgs a;
  a.What = What;
  a.n_rows = n_rows;
  a.cand_idx = cand_idx;
  a.cand_score = cand_score;
  a.n_cand = n_cand;
  a.k = k;
  a.lambda = lambda;
  a.oml = 1.0f - lambda;
  a.out_idx = out_idx;
  a.out_pos = out_pos;
  a.out_score = out_score;
  a.out_pen = out_pen;
  a.err = err_flag;
  int status = ANIREC_OK;
  with_width(dim, [&](auto kd) {
    constexpr int kD = decltype(kd)::value;
    constexpr int kMaxCand = kMmrImageFloats / kD;
    const auto lds = [](int n) { return ((size_t)kD * (n | 1) + 2 * (size_t)n) * sizeof(float); };
    hipError_t e = hipFuncSetAttribute((const void *)k_mmr<kD>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds(kMaxCand));
    if (e == hipSuccess) e = hipMemsetAsync(err_flag, 0, sizeof(int32_t), s);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_mmr<kD>, dim3(n_lists), dim3(kMmrThreads), lds(n_cand), s, a);
      e = hipGetLastError();
    }
    status = (int)e;
  });
  return status;
}

}  // extern "C"
