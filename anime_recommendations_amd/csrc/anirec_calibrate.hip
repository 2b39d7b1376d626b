// Calibrated re-rank of candidate lists for gfx950 (MI355X): include/anirec.h, anirec_calibrate_rerank and
// anirec_list_calibration.  A list of n_cand candidates (rows of the category-bit table, with a relevance score each)
// becomes a list of k picks; each pick maximises  (1 - c) * score - c * (the miscalibration of the list with that
// candidate added): the total variation distance between the category-token distribution of the list and the user's
// favourite profile.  Everything up to one fp64 division is integer arithmetic, so no sum depends on its order.
//   k_calibrate<kWaves>   one group of 64 * kWaves lanes (a whole workgroup) per list, every pick inside the one launch:
//                         kWaves = 1 for n_cand <= 256 (a pick is a wave butterfly, the workgroup barriers of a
//                         one-wave workgroup cost nothing), kWaves = 4 beyond (up to 1024 candidates).
//     check    every index and every profile entry of the list is validated before anything is read through an index
//              (a bad one: the list's outputs become -1 / NaN, *err = 1, nothing gathered).
//     stage    no table rows: lane i owns candidates i, i + 64 kWaves, ... (four at most) and keeps their bit words
//              (1 .. 4), their popcount, score and live state in registers; the words also go to LDS once, so that every
//              lane can read the winner's.  p and q (the profile and the list's counts per category) live in LDS.
//     S0       per pick and per possible popcount t = 0 .. n_cat:  S0[t] = sum_c |p_c (Q + t) - q_c P|, lane t over c
//              (p_c and q_c are broadcast reads): (n_cat + 1) n_cat terms a pick.
//     pick     a candidate's numerator is S0[pop_i] plus, for each of ITS categories, the change of that one term when
//              q_c becomes q_c + 1: pop_i terms.  A term is two 32 x 32 -> 64 multiplies (p_c <= 2^24, Q' < 2^18,
//              q_c <= 1024, P <= 2^31).  pen = (float)((double)num / (double)den), val -> mmr_key packed over ~position,
//              wave butterfly, then kWaves words through LDS.  The owner of the winner writes the four outputs.
//     update   lane c adds the winner's bit c to q_c; Q grows by its popcount.
//   k_list_calibration    one wave per list: the slots' bit words staged in LDS, lane c counts q_c, a wave sum of the
//                         integer terms.
// LDS: n_cand * cat_words words (dynamic; 16 KiB at 1024 x 128) + p, q (1 KiB) + S0 (129 x 8 B) + the wave maxima:
// 3.0 KiB for 100 candidates x 43 categories, 18.3 KiB at most.  No workspace, no atomics; err is a plain store of the
// one value 1.
#include <hip/hip_runtime.h>
#include <math.h>

#include "anirec_dev.hpp"

namespace anirec {

constexpr int kCalMaxCand = 1024;
constexpr int kCalMaxCat = 128;
constexpr int kCalSlots = 4;           // candidates a lane owns at most
constexpr int kCalWords = kCalMaxCat / 32;
constexpr int32_t kCalProfileMax = 1 << 24;

struct CalArgs {
  const uint32_t *cat_bits;   // [n_rows][cw]
  int n_rows, n_cat, cw;
  uint32_t last_mask;         // the bits of the last word below n_cat
  const int32_t *cand_idx;    // [n_lists][n_cand], -1 = empty slot
  const float *cand_score;    // [n_lists][n_cand]
  const int32_t *profile;     // [n_lists][n_cat]
  int n_cand, k;
  float c, omc;               // omc = 1.0f - c
  int32_t *out_idx, *out_pos; // [n_lists][k]
  float *out_score, *out_pen; // [n_lists][k]
  int32_t *err;
};

// |p_c Q' - q_c P|: two 32 x 32 -> 64 products
__device__ __forceinline__ unsigned long long cal_term(uint32_t p, uint32_t Qp, uint32_t q, uint32_t P) {
  const unsigned long long x = (unsigned long long)p * Qp, y = (unsigned long long)q * P;
  return x > y ? x - y : y - x;
}

// the miscalibration from its integer numerator: num, P and Q' are exact in fp64, the division and the conversion to fp32
// each round once
__device__ __forceinline__ float cal_pen(unsigned long long num, uint32_t P, uint32_t Qp) {
  if (P == 0u) return 0.f;
  if (Qp == 0u) return 1.f;
  return (float)((double)num / (double)(2ull * P * Qp));
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int kWaves>
__global__ __launch_bounds__(64 * kWaves) void k_calibrate(CalArgs a) {
  constexpr int kT = 64 * kWaves;
  extern __shared__ __attribute__((aligned(16))) uint32_t cal_smem[];  // [n_cand][cw] the candidates' bit words
  __shared__ uint32_t p_s[kCalMaxCat], q_s[kCalMaxCat];
  __shared__ unsigned long long S0[kCalMaxCat + 1];
  __shared__ unsigned long long best_w[kWaves];
  const int tid = threadIdx.x, n = a.n_cand, k = a.k, cw = a.cw, n_cat = a.n_cat;
  const size_t l = blockIdx.x;
  const int32_t *cidx = a.cand_idx + l * (size_t)n;
  const float *cscore = a.cand_score + l * (size_t)n;
  const int32_t *prof = a.profile + l * (size_t)n_cat;
  int32_t *o_idx = a.out_idx + l * (size_t)k, *o_pos = a.out_pos + l * (size_t)k;
  float *o_score = a.out_score + l * (size_t)k, *o_pen = a.out_pen + l * (size_t)k;
  const float nanv = __uint_as_float(0x7FC00000u);

  // check: nothing is read through an index before every index and profile entry of the list has passed
  int bad = 0;
  int32_t row[kCalSlots];
#pragma unroll
  for (int j = 0; j < kCalSlots; ++j) {
    const int c = tid + j * kT;
    row[j] = -1;
    if (c < n) {
      row[j] = cidx[c];
      bad |= (row[j] < -1 || row[j] >= a.n_rows);
    }
  }
  for (int c = tid; c < n_cat; c += kT) {
    const int32_t v = prof[c];
    bad |= (v < 0 || v > kCalProfileMax);
    p_s[c] = (uint32_t)v;
    q_s[c] = 0u;
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) *a.err = 1;
    for (int s = tid; s < k; s += kT) {
      o_idx[s] = -1;
      o_pos[s] = -1;
      o_score[s] = nanv;
      o_pen[s] = nanv;
    }
    return;
  }
  uint32_t P = 0u;  // <= 128 * 2^24 = 2^31
  for (int c = 0; c < n_cat; ++c) P += p_s[c];

  // stage: the bit words of the lane's own candidates, in registers and (for the update) in LDS
  uint32_t b[kCalSlots][kCalWords];
  uint32_t pop[kCalSlots];
  float sc[kCalSlots], ls[kCalSlots], pen[kCalSlots];
  bool live[kCalSlots];  // present and not yet picked
#pragma unroll
  for (int j = 0; j < kCalSlots; ++j) {
    const int c = tid + j * kT;
    sc[j] = 0.f;
    pop[j] = 0u;
    pen[j] = 0.f;
    live[j] = false;
#pragma unroll
    for (int w = 0; w < kCalWords; ++w) b[j][w] = 0u;
    if (c < n) {
      sc[j] = cscore[c];
      live[j] = row[j] >= 0 && !(sc[j] != sc[j]);
#pragma unroll
      for (int w = 0; w < kCalWords; ++w) {
        if (w < cw) {
          uint32_t x = row[j] >= 0 ? a.cat_bits[(size_t)row[j] * cw + w] : 0u;
          if (w == cw - 1) x &= a.last_mask;
          b[j][w] = x;
          pop[j] += __popc(x);
          cal_smem[c * cw + w] = x;
        }
      }
    }
    ls[j] = mmr_mul(a.omc, sc[j]);
  }

  uint32_t Q = 0u;  // tokens of the picks so far: <= 1024 * 128
  int s = 0;
  for (; s < k; ++s) {
    __syncthreads();  // q_s of this pick (and, the first time, the staged words) are written
    for (int t = tid; t <= n_cat; t += kT) {
      unsigned long long sum = 0ull;
      for (int c = 0; c < n_cat; ++c) sum += cal_term(p_s[c], Q + t, q_s[c], P);
      S0[t] = sum;
    }
    __syncthreads();
    unsigned long long mine = 0ull;
#pragma unroll
    for (int j = 0; j < kCalSlots; ++j) {
      if (!live[j]) continue;
      const uint32_t Qp = Q + pop[j];
      unsigned long long num = S0[pop[j]];
#pragma unroll
      for (int w = 0; w < kCalWords; ++w) {
        uint32_t x = b[j][w];
        while (x) {
          const int c = w * 32 + __ffs(x) - 1;
          x &= x - 1u;
          const uint32_t pc = p_s[c], qc = q_s[c];
          num += cal_term(pc, Qp, qc + 1u, P) - cal_term(pc, Qp, qc, P);  // (mod 2^64: the whole sum is >= 0)
        }
      }
      pen[j] = cal_pen(num, P, Qp);
      const uint32_t c = tid + j * kT;
      const unsigned long long w64 = ((unsigned long long)mmr_key(mmr_val(ls[j], a.c, pen[j])) << 32) | (0xFFFFFFFFu - c);
      mine = w64 > mine ? w64 : mine;
    }
    mine = wave_max_u64(mine);
    if ((tid & 63) == 0) best_w[tid >> 6] = mine;
    __syncthreads();
    unsigned long long best = best_w[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) best = best_w[w] > best ? best_w[w] : best;
    if ((best >> 32) == 0ull) break;  // no present candidate is left (uniform over the workgroup)
    const int pos = (int)(0xFFFFFFFFu - (uint32_t)best);
#pragma unroll
    for (int j = 0; j < kCalSlots; ++j) {
      if (pos == tid + j * kT) {
        o_idx[s] = row[j];
        o_pos[s] = pos;
        o_score[s] = sc[j];
        o_pen[s] = pen[j];
        live[j] = false;
      }
    }
    if (s + 1 == k) continue;
    // update: the winner's categories enter q (every read of q_s for this pick lies before the barrier above)
    const uint32_t *wb = cal_smem + pos * cw;
    for (int c = tid; c < n_cat; c += kT) q_s[c] += (wb[c >> 5] >> (c & 31)) & 1u;
    for (int w = 0; w < cw; ++w) Q += __popc(wb[w]);
  }
  // fewer than k present candidates: the rest of the row
  for (int r = s + tid; r < k; r += kT) {
    o_idx[r] = -1;
    o_pos[r] = -1;
    o_score[r] = nanv;
    o_pen[r] = nanv;
  }
}

struct ListCalArgs {
  const uint32_t *cat_bits;
  int n_rows, n_cat, cw;
  uint32_t last_mask;
  const int32_t *lists;    // [n_lists][k], -1 = empty slot
  const int32_t *profile;  // [n_lists][n_cat]
  int k;
  long long *out_num, *out_den;  // [n_lists]
  float *out_pen;                // [n_lists]
  int32_t *err;
};

__global__ __launch_bounds__(64) void k_list_calibration(ListCalArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cal_smem[];  // [k][cw] the slots' bit words
  const int tid = threadIdx.x, k = a.k, cw = a.cw, n_cat = a.n_cat;
  const size_t l = blockIdx.x;
  const int32_t *list = a.lists + l * (size_t)k;
  const int32_t *prof = a.profile + l * (size_t)n_cat;

  int bad = 0;
  for (int s = tid; s < k; s += 64) {
    const int32_t r = list[s];
    bad |= (r < -1 || r >= a.n_rows);
  }
  uint32_t p[2] = {0u, 0u}, q[2] = {0u, 0u};  // categories tid and tid + 64
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = tid + 64 * j;
    if (c < n_cat) {
      const int32_t v = prof[c];
      bad |= (v < 0 || v > kCalProfileMax);
      p[j] = (uint32_t)v;
    }
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) {
      *a.err = 1;
      a.out_num[l] = -1;
      a.out_den[l] = -1;
      a.out_pen[l] = __uint_as_float(0x7FC00000u);
    }
    return;
  }
  for (int e = tid; e < k * cw; e += 64) {
    const int s = e / cw, w = e - s * cw;
    const int32_t r = list[s];
    uint32_t x = r >= 0 ? a.cat_bits[(size_t)r * cw + w] : 0u;
    if (w == cw - 1) x &= a.last_mask;
    cal_smem[e] = x;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int c = tid + 64 * j;
    if (c < n_cat)
      for (int s = 0; s < k; ++s) q[j] += (cal_smem[s * cw + (c >> 5)] >> (c & 31)) & 1u;
  }
  const uint32_t P = (uint32_t)wave_sum_u64(p[0] + p[1]), Q = (uint32_t)wave_sum_u64(q[0] + q[1]);
  const unsigned long long num = wave_sum_u64(cal_term(p[0], Q, q[0], P) + cal_term(p[1], Q, q[1], P));
  if (tid == 0) {
    const bool degenerate = P == 0u || Q == 0u;  // nothing to calibrate to: 0 / 1; a list that says nothing: 1 / 1
    a.out_num[l] = degenerate ? (P == 0u ? 0 : 1) : (long long)num;
    a.out_den[l] = degenerate ? 1 : (long long)(2ull * P * Q);
    a.out_pen[l] = cal_pen(num, P, Q);
  }
}

static inline uint32_t last_word_mask(int32_t n_cat) { return (n_cat & 31) ? (1u << (n_cat & 31)) - 1u : 0xFFFFFFFFu; }

}  // namespace anirec

using namespace anirec;

extern "C" {

size_t anirec_calibrate_max_cand(void) { return (size_t)kCalMaxCand; }

int anirec_calibrate_rerank(const uint32_t *cat_bits, int32_t n_rows, int32_t n_cat, const int32_t *cand_idx,
                            const float *cand_score, const int32_t *profile, int32_t n_lists, int32_t n_cand, int32_t k,
                            float calibration, int32_t *out_idx, int32_t *out_pos, float *out_score, float *out_pen,
                            int32_t *err_flag, void *stream) {
  if (n_cat < 1 || n_cat > kCalMaxCat || n_rows < 1 || n_lists < 0 || n_cand < 0 || k < 1 || k > n_cand ||
      n_cand > kCalMaxCand || !(calibration >= 0.f && calibration <= 1.f))
    return ANIREC_EINVAL;
  if (n_lists == 0) return ANIREC_OK;
  if (!cat_bits || !cand_idx || !cand_score || !profile || !out_idx || !out_pos || !out_score || !out_pen || !err_flag)
    return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  CalArgs a;
  a.cat_bits = cat_bits;
  a.n_rows = n_rows;
  a.n_cat = n_cat;
  a.cw = (n_cat + 31) / 32;
  a.last_mask = last_word_mask(n_cat);
  a.cand_idx = cand_idx;
  a.cand_score = cand_score;
  a.profile = profile;
  a.n_cand = n_cand;
  a.k = k;
  a.c = calibration;
  a.omc = 1.0f - calibration;
  a.out_idx = out_idx;
  a.out_pos = out_pos;
  a.out_score = out_score;
  a.out_pen = out_pen;
  a.err = err_flag;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, sizeof(int32_t), s));
  const size_t lds = (size_t)n_cand * a.cw * sizeof(uint32_t);
  if (n_cand <= 64 * kCalSlots)
    hipLaunchKernelGGL(k_calibrate<1>, dim3(n_lists), dim3(64), lds, s, a);
  else
    hipLaunchKernelGGL(k_calibrate<4>, dim3(n_lists), dim3(256), lds, s, a);
  return (int)hipGetLastError();
}

int anirec_list_calibration(const uint32_t *cat_bits, int32_t n_rows, int32_t n_cat, const int32_t *lists,
                            const int32_t *profile, int32_t n_lists, int32_t k, int64_t *out_num, int64_t *out_den,
                            float *out_pen, int32_t *err_flag, void *stream) {
  if (n_cat < 1 || n_cat > kCalMaxCat || n_rows < 1 || n_lists < 0 || k < 1 || k > kCalMaxCand) return ANIREC_EINVAL;
  if (n_lists == 0) return ANIREC_OK;
  if (!cat_bits || !lists || !profile || !out_num || !out_den || !out_pen || !err_flag) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ListCalArgs a;
  a.cat_bits = cat_bits;
  a.n_rows = n_rows;
  a.n_cat = n_cat;
  a.cw = (n_cat + 31) / 32;
  a.last_mask = last_word_mask(n_cat);
  a.lists = lists;
  a.profile = profile;
  a.k = k;
  a.out_num = (long long *)out_num;
  a.out_den = (long long *)out_den;
  a.out_pen = out_pen;
  a.err = err_flag;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(k_list_calibration, dim3(n_lists), dim3(64), (size_t)k * a.cw * sizeof(uint32_t), s, a);
  return (int)hipGetLastError();
}

}  // extern "C"
