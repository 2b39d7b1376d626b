// Inference hot path of libanirec for gfx950 (MI355X).
//
//   rownorm        get_weights(): W / ||W||  (similar_anime.py:136-171, similar_users.py:75-101)
//   cosine scores  np.dot(W_hat, W_hat[q])   (similar_anime.py:404, similar_users.py:293)
//   top-k select   np.argsort + slice        (similar_anime.py:408, similar_users.py:294-296,
//                                             model_recs.py:396)
//   predict        model.predict([u, a])     (model_recs.py:394)
//
// Score arithmetic is DEFINED (see oracle/): every dot product is the k-ordered fp32
// fused-multiply-add chain s = fma(x[k], y[k], s), k = 0..127 — the order of
// v_mfma_f32_32x32x2_f32 — so neighbour lists are reproducible bit-for-bit.
#include <hip/hip_runtime.h>
#include <math.h>

#include "anirec_dev.hpp"

namespace anirec {

// ------------------------------------------------------------------------------------
// row normalisation
// ------------------------------------------------------------------------------------
// mode 0: NumPy get_weights  : x / sqrt(sum x^2)            (no epsilon, zero row -> NaN)
// mode 1: tf.nn.l2_normalize : x * (1/sqrt(max(sum x^2, 1e-12)))   (Dot(normalize=True))
// rows: optional gather list (out row j = W[rows[j]]), else identity.
// A row is one group of kD / 4 lanes (a half-wave at 128), 1024 / kD rows per workgroup.

// sum(x^2) of a row in the order NumPy's add.reduce takes over a contiguous fp32 row of kD <= 256 elements (the
// reference's np.linalg.norm(W, axis=1): squares rounded to fp32, then the pairwise sum's unrolled block): eight
// accumulators r[j] = ((x[j] + x[j + 8]) + x[j + 16]) + ... folded in index order over blocks of 128 elements,
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) per block, the two blocks of a 256-wide row added last.  With
// the same sum, the correctly rounded sqrt and divide give NumPy's row bit for bit, whatever the row holds; a
// butterfly order (the 128-wide kernel's, pinned there by its bitwise tests) leaves the norm an ulp away on some
// rows and some quotients three ulps away.  Lane l holds elements 4l .. 4l + 3: even lanes carry r0..r3, odd lanes
// r4..r7, and the fold walks the lanes of equal parity in order — kB / 2 - 1 dependent steps of four shuffles.
template <int kD>
__device__ __forceinline__ float sumsq_numpy_order(const float4 &x, int l) {
#pragma clang fp contract(off)
  constexpr int kG = kD / 4, kB = kG < 32 ? kG : 32;  // lanes of one 128-element block
  const int lb = l & (kB - 1);
  const float4 sq = make_float4(x.x * x.x, x.y * x.y, x.z * x.z, x.w * x.w);
  float4 p = sq;
#pragma unroll
  for (int s = 2; s < kB; s += 2) {
    float4 up;
    up.x = __shfl_up(p.x, 2, kG);
    up.y = __shfl_up(p.y, 2, kG);
    up.z = __shfl_up(p.z, 2, kG);
    up.w = __shfl_up(p.w, 2, kG);
    if ((lb & ~1) == s) p = make_float4(up.x + sq.x, up.y + sq.y, up.z + sq.z, up.w + sq.w);
  }
  const float h = (p.x + p.y) + (p.z + p.w);
  float ss = __shfl(h, kB - 2, kG) + __shfl(h, kB - 1, kG);
  if constexpr (kG > kB) ss = ss + (__shfl(h, kB + kB - 2, kG) + __shfl(h, kB + kB - 1, kG));
  return ss;
}

template <int kMode, int kD>
__device__ __forceinline__ void rownorm_body(const float *W, const int32_t *rows, int n, float *out) {
  constexpr int kG = kD / 4, kRpb = 256 / kG;
  const int l = threadIdx.x & (kG - 1);
  const int nhw = gridDim.x * kRpb;
  for (int r = blockIdx.x * kRpb + (threadIdx.x / kG); r < n; r += nhw) {
    const int src = rows ? rows[r] : r;
    float4 x = reinterpret_cast<const float4 *>(W)[(size_t)src * kG + l];
    float ss;
    if constexpr (kMode == 0 && kD != kDim) {
      ss = sumsq_numpy_order<kD>(x, l);
    } else {
      ss = x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
      ss = group_sum<kG>(ss);
    }
    float4 y;
    if (kMode == 0) {
      const float nrm = sqrtf(ss);
      y.x = x.x / nrm;
      y.y = x.y / nrm;
      y.z = x.z / nrm;
      y.w = x.w / nrm;
    } else {
      const float rinv = 1.0f / sqrtf(fmaxf(ss, kL2nEps));
      y.x = x.x * rinv;
      y.y = x.y * rinv;
      y.z = x.z * rinv;
      y.w = x.w * rinv;
    }
    reinterpret_cast<float4 *>(out)[(size_t)r * kG + l] = y;
  }
}
template <int kMode, int kD = kDim>
__global__ __launch_bounds__(256) void k_rownorm(const float *W, const int32_t *rows, int n, float *out) {
  rownorm_body<kMode, kD>(W, rows, n, out);
}
template <int kMode>
static void launch_rownorm(const float *W, const int32_t *rows, int n, float *out, int dim, hipStream_t s) {
  int blocks = (int)(((long long)n * dim + 1023) / 1024);  // 1024 / dim rows per workgroup
  if (blocks > 4096) blocks = 4096;
  with_width(dim, [&](auto kd) {
    hipLaunchKernelGGL((k_rownorm<kMode, decltype(kd)::value>), dim3(blocks), dim3(256), 0, s, W, rows, n, out);
  });
}
// the mode-1 rows for the other translation units (anirec_foldin.hip): the same kernels, nothing instantiated twice
void l2norm_rows(const float *W, int n, float *out, int dim, hipStream_t s) {
  launch_rownorm<1>(W, nullptr, n, out, dim, s);
}

// ------------------------------------------------------------------------------------
// tiled scores: out[q][j] = epilogue( chain_dot(Q[q], W[j]) )
// 64 queries x 64 rows per workgroup, 4x4 register block per thread, both tiles staged
// in LDS with a 132-float row pitch (ds_read_b128 of rows tx+16r is conflict-free).
// ------------------------------------------------------------------------------------
constexpr int kTile = 64;
// floats of a row staged in LDS at a time: the whole row up to 128 (pitch 132: the two 64-row tiles take 66 KB); a
// 256-wide row is walked in two 128-float slices, the fma chain running on through both
template <int kD>
struct ScoreGeom {
  static constexpr int kS = kD < kDim ? kD : kDim;  // floats per slice
  static constexpr int kSV = kS / 4, kPitch = kS + 4, kRowV = kD / 4;
};

struct ScoreArgs {
  const float *Q;         // [*, dim] query matrix
  const int32_t *qrows;   // optional: query j reads Q[qrows[j]]
  int nq;
  const float *W;         // [n, dim]
  int n;
  float *out;             // [nq][ld]
  size_t ld;
  int use_head;           // 1: act(c*hs + hb), the kernel's activation kAct
  float hs, hb;
  int act;                // the activation as a run-time value: read by the kernels of the other widths only
};

// kAct >= 0: the activation of the epilogue as a template parameter (k_scores: the 128-wide kernel); < 0: a.act
template <int kAct, int kD>
__device__ __forceinline__ void scores_body(const ScoreArgs &a) {
  constexpr int kSV = ScoreGeom<kD>::kSV, kPitch = ScoreGeom<kD>::kPitch, kRowV = ScoreGeom<kD>::kRowV;
  __shared__ __attribute__((aligned(16))) float Qs[kTile * kPitch];
  __shared__ __attribute__((aligned(16))) float Ws[kTile * kPitch];
  const int tid = threadIdx.x;
  const int q0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
  const int tx = tid & 15, ty = tid >> 4;  // rows tx+16r, queries ty+16q
  float acc[4][4];
#pragma unroll
  for (int qq = 0; qq < 4; ++qq)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[qq][r] = 0.f;
#pragma unroll
  for (int k0 = 0; k0 < kRowV; k0 += kSV) {  // (one pass up to 128)
    if (k0) __syncthreads();                 // the previous slice has been read
    // stage: 64 rows x kSV float4 per tile (128: 32 float4 a row, 8 per thread and tile)
    for (int e = tid; e < kTile * kSV; e += 256) {
      const int r = e / kSV, cidx = e % kSV;
      float4 qv = make_float4(0.f, 0.f, 0.f, 0.f), wv = qv;
      if (q0 + r < a.nq) {
        const int src = a.qrows ? a.qrows[q0 + r] : q0 + r;
        qv = reinterpret_cast<const float4 *>(a.Q)[(size_t)src * kRowV + k0 + cidx];
      }
      if (j0 + r < a.n) wv = reinterpret_cast<const float4 *>(a.W)[(size_t)(j0 + r) * kRowV + k0 + cidx];
      *reinterpret_cast<float4 *>(&Qs[r * kPitch + cidx * 4]) = qv;
      *reinterpret_cast<float4 *>(&Ws[r * kPitch + cidx * 4]) = wv;
    }
    __syncthreads();
#pragma unroll 4
    for (int k4 = 0; k4 < kSV; ++k4) {
      float4 qv[4], wv[4];
#pragma unroll
      for (int qq = 0; qq < 4; ++qq)
        qv[qq] = *reinterpret_cast<const float4 *>(&Qs[(ty + 16 * qq) * kPitch + k4 * 4]);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        wv[r] = *reinterpret_cast<const float4 *>(&Ws[(tx + 16 * r) * kPitch + k4 * 4]);
#pragma unroll
      for (int qq = 0; qq < 4; ++qq)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float s = acc[qq][r];
          s = __fmaf_rn(wv[r].x, qv[qq].x, s);
          s = __fmaf_rn(wv[r].y, qv[qq].y, s);
          s = __fmaf_rn(wv[r].z, qv[qq].z, s);
          s = __fmaf_rn(wv[r].w, qv[qq].w, s);
          acc[qq][r] = s;
        }
    }
  }
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) {
    const int q = q0 + ty + 16 * qq;
    if (q >= a.nq) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = j0 + tx + 16 * r;
      if (j >= a.n) continue;
      float s = acc[qq][r];
      if (a.use_head) s = rating_from_cosine<kAct>(s, a.hs, a.hb, a.act);
      a.out[(size_t)q * a.ld + j] = s;
    }
  }
}

template <int kAct>
__global__ __launch_bounds__(256) void k_scores(ScoreArgs a) {
  scores_body<kAct, kDim>(a);
}
template <int kD>  // the widths other than 128, any activation (a.act)
__global__ __launch_bounds__(256) void k_scores_w(ScoreArgs a) {
  scores_body<-1, kD>(a);
}

// ------------------------------------------------------------------------------------
// exact top-k of each score row: 4-pass MSB radix select on order-preserving keys, then
// ordered collection (ties -> ascending index) and a bitonic sort of the k winners.
// ------------------------------------------------------------------------------------
// (the key of a score, score_key, is in anirec_dev.hpp: the fusion of anirec_fuse.hip orders by it too)
struct SelectArgs {
  const float *scores;   // [nq][ld]
  size_t ld;
  int n, nq, k;
  const int32_t *self;   // optional [nq]: index excluded for query q (or -1)
  const uint8_t *keep;   // optional [n] byte mask shared by all queries
  const uint32_t *wbits; // optional [nq][wwords] bit mask: set bit = excluded (watched)
  int wwords;
  int32_t *out_idx;      // [nq * slices][k]
  float *out_score;      // [nq * slices][k]
  int slices, slice_len; // workgroup b selects among keys [s*slice_len, (s+1)*slice_len) of query b / slices
  const int32_t *src_idx; // merge pass: [nq][ld] real index of list entry j (-1 = empty), masks already applied
};

__device__ __forceinline__ uint32_t cand_key(const SelectArgs &a, const float *row, int q, int j,
                                             int self) {
  if (a.src_idx) return a.src_idx[(size_t)q * a.ld + j] < 0 ? 0u : score_key(row[j]);
  if (j == self) return 0u;
  if (a.keep && !a.keep[j]) return 0u;
  if (a.wbits && ((a.wbits[(size_t)q * a.wwords + (j >> 5)] >> (j & 31)) & 1u)) return 0u;
  return score_key(row[j]);
}

constexpr int kSelThreads = 256;

// ---- the select body, once: k_select collects into its LDS window, the any-k kernels (k_lk_*, further down) into
// global rows.  The tie rule, the short-row rule and the eq_use accounting live here and nowhere else. ----

// The digit of one radix pass from a 256-bin histogram in LDS: the digit d (from 255 down) where the running count
// first reaches `want`, by a wave scan instead of a 256-step serial walk by one thread (that walk was ~8 us per pass:
// most of a small select).  out[0], out[1] = the new prefix and want, or 0xFFFFFFFF and 0 when fewer than `want` keys
// match (pass 0 only: fewer than k candidates); out[2] = the keys matching the prefix.  Ends with a barrier.
__device__ void sel_digit(const uint32_t *hist, uint32_t prefix, uint32_t want, int shift, uint32_t *out) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    uint32_t h4[4], run = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // lane l covers digits 255-4l .. 252-4l, in that order
      h4[j] = hist[255 - (4 * tid + j)];
      run += h4[j];
    }
    uint32_t inc = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(inc, o, 64);
      if (tid >= o) inc += y;
    }
    const uint32_t before = inc - run;  // candidates in digits above this lane's four
    const unsigned long long reach = __ballot(inc >= want);
    if (tid == 63) out[2] = inc;
    if (reach == 0ull) {
      if (tid == 0) {  // fewer than k candidates in total: take them all
        out[0] = 0xFFFFFFFFu;
        out[1] = 0;
      }
    } else if (tid == __ffsll((long long)reach) - 1) {
      uint32_t cum = before;
      int j = 0;
      for (; j < 3; ++j) {
        if (cum + h4[j] >= want) break;
        cum += h4[j];
      }
      out[0] = prefix | ((uint32_t)(255 - (4 * tid + j)) << shift);
      out[1] = want - cum;
    }
  }
  __syncthreads();
}

// hist[d] = candidates of [j_lo, j_hi) whose key matches `prefix` under `pmask` and has digit d at `shift`
__device__ void sel_hist(const SelectArgs &a, const float *row, int q, int self, int j_lo, int j_hi, uint32_t prefix,
                         uint32_t pmask, int shift, uint32_t *hist) {
  const int tid = threadIdx.x;
  hist[tid] = 0;
  __syncthreads();
  for (int j = j_lo + tid; j < j_hi; j += kSelThreads) {
    const uint32_t key = cand_key(a, row, q, j, self);
    if (key != 0u && (key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
  }
  __syncthreads();
}

__device__ __forceinline__ uint32_t sel_pmask(int pass) { return pass == 0 ? 0u : 0xFFFFFFFFu << (32 - 8 * pass); }

// state (prefix, want, m, short) after pass p from the one after pass p - 1 and the digit scan of pass p
__device__ uint4 sel_advance(uint4 prev, const uint32_t *sh) {
  if (sh[0] == 0xFFFFFFFFu && sh[1] == 0) return make_uint4(0u, 0xFFFFFFFFu, sh[2], 1u);
  return make_uint4(sh[0], sh[1], prev.z, 0u);
}

// Ordered collection of the winners of [j_lo, j_hi) into w[0..cap): every key > T and the first `need_eq` keys == T in
// ascending index order; short_row: every candidate.  n_out / eq_taken: winners / keys == T already taken by the
// slices before this one.  w is k_select's LDS window or a global row.
__device__ void sel_collect(const SelectArgs &a, const float *row, int q, int self, int j_lo, int j_hi, uint32_t T,
                            uint32_t need_eq, bool short_row, uint32_t n_out, uint32_t eq_taken,
                            unsigned long long *w, uint32_t cap, uint32_t *wsum) {
  const int tid = threadIdx.x;
  constexpr int kPer = 16;
  const int super = kSelThreads * kPer;
  for (int base = j_lo; base < j_hi; base += super) {
    uint32_t keys[kPer];
    uint32_t c_gt = 0, c_eq = 0;
    const int j0 = base + tid * kPer;
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      const int j = j0 + e;
      keys[e] = j < j_hi ? cand_key(a, row, q, j, self) : 0u;
      if (keys[e] != 0u) {
        if (short_row || keys[e] > T) ++c_gt;
        else if (keys[e] == T) ++c_eq;
      }
    }
    if (__syncthreads_count((c_gt | c_eq) != 0) == 0) continue;
    // ordered ranks of this thread's matches: counts can reach 4096 per super-chunk -> two separate scans
    uint32_t tot_gt = 0, tot_eq = 0;
    uint32_t o_gt, o_eq;
    {
      const int lane = tid & 63, wv = tid >> 6;
      uint32_t inc = c_gt;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
      }
      if (lane == 63) wsum[wv] = inc;
      __syncthreads();
      uint32_t b = 0;
      for (int kk = 0; kk < kSelThreads / 64; ++kk) {
        if (kk < wv) b += wsum[kk];
        tot_gt += wsum[kk];
      }
      o_gt = b + inc - c_gt;
      __syncthreads();
      inc = c_eq;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
      }
      if (lane == 63) wsum[wv] = inc;
      __syncthreads();
      b = 0;
      for (int kk = 0; kk < kSelThreads / 64; ++kk) {
        if (kk < wv) b += wsum[kk];
        tot_eq += wsum[kk];
      }
      o_eq = b + inc - c_eq;
      __syncthreads();
    }
    const uint32_t eq_room = need_eq == 0xFFFFFFFFu ? 0u : (need_eq - eq_taken);
    const uint32_t eq_use = tot_eq < eq_room ? tot_eq : eq_room;
    // winners land at [n_out, n_out + tot_gt) for gt and after them the eq ones of this chunk
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
      const uint32_t key = keys[e];
      if (key == 0u) continue;
      const int j = j0 + e;
      if (short_row || key > T) {
        const uint32_t slot = n_out + o_gt++;
        if (slot < cap) w[slot] = ((unsigned long long)key << 32) | (uint32_t)(~(uint32_t)j);
      } else if (key == T) {
        const uint32_t r = o_eq++;
        if (r < eq_use) {
          const uint32_t slot = n_out + tot_gt + r;
          if (slot < cap) w[slot] = ((unsigned long long)key << 32) | (uint32_t)(~(uint32_t)j);
        }
      }
    }
    n_out += tot_gt + eq_use;
    eq_taken += eq_use;
  }
}

__global__ __launch_bounds__(kSelThreads) void k_select(SelectArgs a) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sh[3];
  __shared__ uint32_t wsum[kSelThreads / 64];
  __shared__ unsigned long long win[ANIREC_MAX_TOPK];  // (key << 32) | ~idx  -> sort desc
  const int tid = threadIdx.x;
  // Few queries (the reference's literal call is ONE query against every row): a query's keys are cut
  // into slices, one workgroup each, and a second launch of this kernel merges the slice winners.  The
  // winners of a slice are sorted (score desc, index asc) and slices cover ascending index ranges, so
  // list order among equal scores is ascending index — the tie rule survives the merge unchanged.
  const int q = blockIdx.x / a.slices;
  const int j_lo = (blockIdx.x % a.slices) * a.slice_len;
  const int j_hi = min(a.n, j_lo + a.slice_len);
  const size_t orow = blockIdx.x;
  const float *row = a.scores + (size_t)q * a.ld;
  const int self = a.self ? a.self[q] : -1;
  const int k = a.k;

  // MSB-first radix select for the k-th largest key among candidates (key != 0)
  uint4 st = make_uint4(0u, (uint32_t)k, (uint32_t)k, 0u);  // prefix, rank still to locate in it, winners, short row
  for (int pass = 0; pass < 4 && !st.w; ++pass) {
    sel_hist(a, row, q, self, j_lo, j_hi, st.x, sel_pmask(pass), 24 - 8 * pass, hist);
    sel_digit(hist, st.x, st.y, 24 - 8 * pass, sh);
    st = sel_advance(st, sh);
    __syncthreads();
  }
  // threshold T = prefix (exact key of the k-th largest); take all keys > T and the first
  // `want` keys == T in ascending index order.  short row: take every candidate.
  sel_collect(a, row, q, self, j_lo, j_hi, st.w ? 0u : st.x, st.w ? 0xFFFFFFFFu : st.y, st.w != 0, 0, 0, win,
              ANIREC_MAX_TOPK, wsum);
  const uint32_t n_out = min(st.z, (uint32_t)ANIREC_MAX_TOPK);
  __syncthreads();
  // pad to 128 with zeros (sort last) and bitonic sort descending
  for (int i = tid; i < ANIREC_MAX_TOPK; i += kSelThreads)
    if ((uint32_t)i >= n_out) win[i] = 0ull;
  __syncthreads();
  for (int size = 2; size <= ANIREC_MAX_TOPK; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (tid < ANIREC_MAX_TOPK / 2) {
        const int lo = 2 * tid - (tid & (stride - 1));
        const int hi = lo + stride;
        const bool desc = ((lo & size) == 0);
        const unsigned long long x = win[lo], y = win[hi];
        if ((x < y) == desc) {
          win[lo] = y;
          win[hi] = x;
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < k; i += kSelThreads) {
    const unsigned long long v = win[i];
    if ((uint32_t)i < n_out && v != 0ull) {
      const int j = (int)(~(uint32_t)(v & 0xFFFFFFFFull));
      a.out_idx[orow * k + i] = a.src_idx ? a.src_idx[(size_t)q * a.ld + j] : j;
      a.out_score[orow * k + i] = row[j];
    } else {
      a.out_idx[orow * k + i] = -1;
      a.out_score[orow * k + i] = __uint_as_float(0x7FC00000u);
    }
  }
}

// ------------------------------------------------------------------------------------
// predict on explicit pairs (model.predict([user_arr, anime_arr]))
// ------------------------------------------------------------------------------------
// a row group (kD / 4 lanes) per pair; kAct < 0: the run-time activation `act`
template <int kAct, int kD>
__device__ __forceinline__ void predict_pairs_body(const float *U, const float *A, const int32_t *ui,
                                                   const int32_t *ai, int n, float hs, float hb, int act, float *p) {
  constexpr int kG = kD / 4;
  const int l = threadIdx.x & (kG - 1);
  const int i = blockIdx.x * (256 / kG) + (threadIdx.x / kG);
  if (i >= n) return;
  const float4 u = reinterpret_cast<const float4 *>(U)[(size_t)ui[i] * kG + l];
  const float4 x = reinterpret_cast<const float4 *>(A)[(size_t)ai[i] * kG + l];
  const float su = group_sum<kG>(u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w);
  const float sa = group_sum<kG>(x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w);
  const float dd = group_sum<kG>(u.x * x.x + u.y * x.y + u.z * x.z + u.w * x.w);
  if (l == 0) {
    const float ru = 1.0f / sqrtf(fmaxf(su, kL2nEps));
    const float ra = 1.0f / sqrtf(fmaxf(sa, kL2nEps));
    p[i] = act_any<kAct>(dd * ru * ra * hs + hb, act);
  }
}
template <int kAct>
__global__ __launch_bounds__(256) void k_predict_pairs(const float *U, const float *A,
                                                       const int32_t *ui, const int32_t *ai, int n,
                                                       float hs, float hb, float *p) {
  predict_pairs_body<kAct, kDim>(U, A, ui, ai, n, hs, hb, 0, p);
}
template <int kD>
__global__ __launch_bounds__(256) void k_predict_pairs_w(const float *U, const float *A, const int32_t *ui,
                                                         const int32_t *ai, int n, float hs, float hb, int act,
                                                         float *p) {
  predict_pairs_body<-1, kD>(U, A, ui, ai, n, hs, hb, act, p);
}

__global__ void k_fill_self(const int32_t *queries, int nq, int32_t *self, int enable) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nq) self[i] = enable ? queries[i] : -1;
}

static inline void head_affine(const anirec_head *h, float *hs, float *hb) { head_affine_f32(h, hs, hb); }

// Few queries (<= 16; the reference's literal call has ONE): a GEMV-shaped kernel.  A workgroup stages 64 key
// rows coalesced into LDS (pitch 132 floats: float4 rows whose 16-lane read groups fall on distinct banks) and
// each thread runs the DEFINED k-ordered fma chain of one (key, query) pair — the same arithmetic as k_scores,
// bit for bit — so the 64 x 64 tile kernel's 63/64 wasted lanes disappear and the pass is HBM-bound.
constexpr int kFewQ = 16;
// Rows are staged a slice (ScoreGeom) at a time.  At 256 a (key, query) pair's chain value waits in its own output
// element between the two slices: written and read back by the same thread, it goes on bit for bit.
template <int kAct, int kD>
__device__ __forceinline__ void scores_few_body(const ScoreArgs &a) {
  constexpr int kS = ScoreGeom<kD>::kS, kSV = ScoreGeom<kD>::kSV, kFewPitch = ScoreGeom<kD>::kPitch,
                kRowV = ScoreGeom<kD>::kRowV;
  __shared__ __attribute__((aligned(16))) float Ws[64 * kFewPitch];
  __shared__ __attribute__((aligned(16))) float Qs[kFewQ * kS];
  const int tid = threadIdx.x;
  const int j0 = blockIdx.x * 64;
  const int key = tid & 63, j = j0 + key;
#pragma unroll
  for (int k0 = 0; k0 < kRowV; k0 += kSV) {  // (one pass up to 128)
    if (k0) __syncthreads();
    for (int e = tid; e < 64 * kSV; e += 256) {
      const int r = e / kSV, c = e % kSV;
      float4 wv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j0 + r < a.n) wv = reinterpret_cast<const float4 *>(a.W)[(size_t)(j0 + r) * kRowV + k0 + c];
      *reinterpret_cast<float4 *>(&Ws[r * kFewPitch + c * 4]) = wv;
    }
    for (int e = tid; e < a.nq * kSV; e += 256) {
      const int q = e / kSV, c = e % kSV;
      const size_t src = a.qrows ? (size_t)a.qrows[q] : (size_t)q;
      *reinterpret_cast<float4 *>(&Qs[q * kS + c * 4]) = reinterpret_cast<const float4 *>(a.Q)[src * kRowV + k0 + c];
    }
    __syncthreads();
    for (int q = tid >> 6; q < a.nq; q += 4) {
      const float4 *w4 = reinterpret_cast<const float4 *>(&Ws[key * kFewPitch]);
      const float4 *q4 = reinterpret_cast<const float4 *>(&Qs[q * kS]);
      float s = 0.f;
      if (k0 && j < a.n) s = a.out[(size_t)q * a.ld + j];
#pragma unroll 8
      for (int k4 = 0; k4 < kSV; ++k4) {
        const float4 x = w4[k4], y = q4[k4];
        s = __fmaf_rn(x.x, y.x, s);
        s = __fmaf_rn(x.y, y.y, s);
        s = __fmaf_rn(x.z, y.z, s);
        s = __fmaf_rn(x.w, y.w, s);
      }
      if (k0 + kSV >= kRowV && a.use_head) s = rating_from_cosine<kAct>(s, a.hs, a.hb, a.act);
      if (j < a.n) a.out[(size_t)q * a.ld + j] = s;
    }
  }
}
template <int kAct>
__global__ __launch_bounds__(256) void k_scores_few(ScoreArgs a) {
  scores_few_body<kAct, kDim>(a);
}
template <int kD>
__global__ __launch_bounds__(256) void k_scores_few_w(ScoreArgs a) {
  scores_few_body<-1, kD>(a);
}

// scratch of the sliced select: at most kSelMaxBlocks slice winners lists of ANIREC_MAX_TOPK entries
constexpr int kSelMaxBlocks = 2048;
constexpr size_t kSelTmpBytes = (size_t)kSelMaxBlocks * ANIREC_MAX_TOPK * 8;

// Few queries (the reference's literal call has ONE) against many keys: a query's keys are cut into S slices, one
// workgroup each, so that the select fills the chip.  The one rule of k_select's launches and of the any-k ones.
static int select_slices(int nq, int n) {
  if (nq >= 1024 || n < 4096) return 1;
  int S = n / 2048;
  if (S > 64) S = 64;
  if (S > kSelMaxBlocks / nq) S = kSelMaxBlocks / nq;
  return S < 1 ? 1 : S;
}

// one launch when there are enough queries to fill the chip; otherwise slices + merge
static int launch_select(SelectArgs sa, void *tmp, hipStream_t s) {
  sa.src_idx = nullptr;
  const int S = select_slices(sa.nq, sa.n);
  sa.slices = S;
  sa.slice_len = (sa.n + S - 1) / S;
  if (S == 1) {
    hipLaunchKernelGGL(k_select, dim3(sa.nq), dim3(kSelThreads), 0, s, sa);
    return (int)hipGetLastError();
  }
  int32_t *tmp_idx = (int32_t *)tmp;
  float *tmp_score = (float *)((char *)tmp + (size_t)kSelMaxBlocks * ANIREC_MAX_TOPK * 4);
  SelectArgs part = sa;
  part.out_idx = tmp_idx;
  part.out_score = tmp_score;
  hipLaunchKernelGGL(k_select, dim3(sa.nq * S), dim3(kSelThreads), 0, s, part);
  SelectArgs m = sa;
  m.scores = tmp_score;
  m.src_idx = tmp_idx;
  m.ld = (size_t)S * sa.k;
  m.n = S * sa.k;
  m.self = nullptr;
  m.keep = nullptr;
  m.wbits = nullptr;
  m.slices = 1;
  m.slice_len = m.n;
  hipLaunchKernelGGL(k_select, dim3(sa.nq), dim3(kSelThreads), 0, s, m);
  return (int)hipGetLastError();
}

// act: the activation of a head (use_head != 0); plain cosine scores take the default instantiation.  dim: the row
// width of a.Q and a.W
static int launch_scores(const ScoreArgs &a0, hipStream_t s, int32_t act = ANIREC_ACT_SIGMOID, int dim = kDim) {
  ScoreArgs a = a0;
  a.act = act;
  if (dim != kDim) {
    with_width(dim, [&](auto kd) {
      constexpr int kD = decltype(kd)::value;
      if constexpr (kD != kDim) {  // (nothing of the run-time-head kernels is instantiated at 128)
        if (a.nq <= kFewQ) {
          hipLaunchKernelGGL(k_scores_few_w<kD>, dim3((a.n + 63) / 64), dim3(256), 0, s, a);
        } else {
          dim3 grid((a.n + kTile - 1) / kTile, (a.nq + kTile - 1) / kTile);
          hipLaunchKernelGGL(k_scores_w<kD>, grid, dim3(256), 0, s, a);
        }
      }
    });
    return (int)hipGetLastError();
  }
  with_act(act, [&](auto k) {
    constexpr int kAct = decltype(k)::value;
    if (a.nq <= kFewQ) {
      hipLaunchKernelGGL(k_scores_few<kAct>, dim3((a.n + 63) / 64), dim3(256), 0, s, a);
    } else {
      dim3 grid((a.n + kTile - 1) / kTile, (a.nq + kTile - 1) / kTile);
      hipLaunchKernelGGL(k_scores<kAct>, grid, dim3(256), 0, s, a);
    }
  });
  return (int)hipGetLastError();
}

// The head of every predict workspace: Ah | Uh, the tf.nn.l2_normalize rows of A and of the call's users.
static size_t norm_bytes(int32_t n_anime, int32_t n_users, int32_t dim) {
  return ((size_t)n_anime + (size_t)n_users) * dim * 4;
}
struct NormRows {
  float *Ah, *Uh;
};
static hipError_t normalise_tables(const float *U, const float *A, int32_t dim, int32_t n_anime, const int32_t *users,
                                   int32_t n_users, void *workspace, hipStream_t s, NormRows *r) {
  r->Ah = (float *)workspace;
  r->Uh = r->Ah + (size_t)n_anime * dim;
  launch_rownorm<1>(A, nullptr, n_anime, r->Ah, dim, s);
  launch_rownorm<1>(U, users, n_users, r->Uh, dim, s);
  return hipGetLastError();
}

}  // namespace anirec

using namespace anirec;

extern "C" {

// Every entry point without a `dim` is its _w twin at ANIREC_DIM.
int anirec_rownorm(const float *W, int32_t n, float *What, void *stream) {
  return anirec_rownorm_w(W, n, ANIREC_DIM, What, stream);
}

int anirec_rownorm_w(const float *W, int32_t n, int32_t dim, float *What, void *stream) {
  if (!W || !What || n < 0 || !dim_ok(dim)) return ANIREC_EINVAL;
  if (n == 0) return ANIREC_OK;
  launch_rownorm<0>(W, nullptr, n, What, dim, (hipStream_t)stream);
  return (int)hipGetLastError();
}

int anirec_cosine_scores(const float *What, int32_t n, int32_t q, float *scores, void *stream) {
  return anirec_cosine_scores_w(What, n, ANIREC_DIM, q, scores, stream);
}

int anirec_cosine_scores_w(const float *What, int32_t n, int32_t dim, int32_t q, float *scores, void *stream) {
  if (!What || !scores || n < 1 || q < 0 || q >= n || !dim_ok(dim)) return ANIREC_EINVAL;
  ScoreArgs a;
  a.Q = What + (size_t)q * dim;
  a.qrows = nullptr;
  a.nq = 1;
  a.W = What;
  a.n = n;
  a.out = scores;
  a.ld = (size_t)n;
  a.use_head = 0;
  a.hs = a.hb = 0.f;
  return launch_scores(a, (hipStream_t)stream, ANIREC_ACT_SIGMOID, dim);
}

// the same kernels on two tables of rows that need not be normalised: one chain, one body
int anirec_dot_scores(const float *Q, int32_t n_q, const float *Y, int32_t n, int32_t dim, float *out, int64_t ld,
                      void *stream) {
  if (n < 1 || n_q < 0 || n_q > 65535 * kTile || ld < n || !dim_ok(dim)) return ANIREC_EINVAL;
  if (n_q == 0) return ANIREC_OK;
  if (!Q || !Y || !out) return ANIREC_EINVAL;
  ScoreArgs a;
  a.Q = Q;
  a.qrows = nullptr;
  a.nq = n_q;
  a.W = Y;
  a.n = n;
  a.out = out;
  a.ld = (size_t)ld;
  a.use_head = 0;
  a.hs = a.hb = 0.f;
  return launch_scores(a, (hipStream_t)stream, ANIREC_ACT_SIGMOID, dim);
}

int anirec_predict_pairs_act(const float *U, const float *A, const int32_t *user_idx,
                             const int32_t *anime_idx, int32_t n, const anirec_head *head, int32_t activation,
                             float *p, void *stream) {
  return anirec_predict_pairs_w(U, A, ANIREC_DIM, user_idx, anime_idx, n, head, activation, p, stream);
}

int anirec_predict_pairs_w(const float *U, const float *A, int32_t dim, const int32_t *user_idx,
                           const int32_t *anime_idx, int32_t n, const anirec_head *head, int32_t activation,
                           float *p, void *stream) {
  if (!U || !A || !user_idx || !anime_idx || !head || !p || n < 0 || !act_ok(activation) || !dim_ok(dim))
    return ANIREC_EINVAL;
  if (n == 0) return ANIREC_OK;
  float hs, hb;
  head_affine(head, &hs, &hb);
  if (dim != kDim) {
    with_width(dim, [&](auto kd) {
      constexpr int kD = decltype(kd)::value, kRpb = 1024 / kD;
      if constexpr (kD != kDim)  // (nothing of k_predict_pairs_w is instantiated at 128)
        hipLaunchKernelGGL(k_predict_pairs_w<kD>, dim3((n + kRpb - 1) / kRpb), dim3(256), 0, (hipStream_t)stream, U, A,
                           user_idx, anime_idx, n, hs, hb, (int)activation, p);
    });
    return (int)hipGetLastError();
  }
  with_act(activation, [&](auto k) {
    hipLaunchKernelGGL(k_predict_pairs<decltype(k)::value>, dim3((n + 7) / 8), dim3(256), 0, (hipStream_t)stream, U, A,
                       user_idx, anime_idx, n, hs, hb, p);
  });
  return (int)hipGetLastError();
}

int anirec_predict_pairs(const float *U, const float *A, const int32_t *user_idx,
                         const int32_t *anime_idx, int32_t n, const anirec_head *head, float *p,
                         void *stream) {
  return anirec_predict_pairs_act(U, A, user_idx, anime_idx, n, head, ANIREC_ACT_SIGMOID, p, stream);
}

int anirec_predict_grid(const float *U, const float *A, int32_t n_anime, const int32_t *users,
                        int32_t n_users, const anirec_head *head, float *out, void *workspace,
                        size_t workspace_bytes, void *stream) {
  return anirec_predict_grid_act(U, A, n_anime, users, n_users, head, ANIREC_ACT_SIGMOID, out, workspace,
                                 workspace_bytes, stream);
}

int anirec_predict_grid_act(const float *U, const float *A, int32_t n_anime, const int32_t *users,
                            int32_t n_users, const anirec_head *head, int32_t activation, float *out,
                            void *workspace, size_t workspace_bytes, void *stream) {
  return anirec_predict_grid_w(U, A, ANIREC_DIM, n_anime, users, n_users, head, activation, out, workspace,
                               workspace_bytes, stream);
}

int anirec_predict_grid_w(const float *U, const float *A, int32_t dim, int32_t n_anime, const int32_t *users,
                          int32_t n_users, const anirec_head *head, int32_t activation, float *out,
                          void *workspace, size_t workspace_bytes, void *stream) {
  if (!U || !A || !users || !head || !out || !workspace || n_anime < 1 || n_users < 0 || !act_ok(activation) ||
      !dim_ok(dim))
    return ANIREC_EINVAL;
  if (n_users == 0) return ANIREC_OK;
  if (workspace_bytes < norm_bytes(n_anime, n_users, dim)) return ANIREC_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  NormRows t;
  ANIREC_HIP_CHECK(normalise_tables(U, A, dim, n_anime, users, n_users, workspace, s, &t));
  ScoreArgs a;
  a.Q = t.Uh;
  a.qrows = nullptr;
  a.nq = n_users;
  a.W = t.Ah;
  a.n = n_anime;
  a.out = out;
  a.ld = (size_t)n_anime;
  a.use_head = 1;
  head_affine(head, &a.hs, &a.hb);
  return launch_scores(a, s, activation, dim);
}

}  // extern "C"

// ====================================================================================
// exact top-k for ANY k (anirec_cosine_topk_large, anirec_predict_topk_large_act)
//
// The same score rows (k_scores / k_scores_few through launch_scores), the same keys (cand_key) and the same select
// body (sel_hist / sel_digit / sel_advance / sel_collect, above k_select) as k_select, so the result is k_select's
// for k <= ANIREC_MAX_TOPK.  Phases, all stream-ordered launches:
//   select   the 4-pass MSB radix select (sel_hist + sel_digit) -> threshold key T, `want` keys == T to take (first
//            in index order), m = winners (k, or every candidate of a short row).  Few queries (select_slices): the
//            histograms of each pass are built per slice by one workgroup each (k_lk_hist) and summed by the next
//            launch; many queries: one workgroup per query does all four passes (k_lk_select_row).
//   collect  the m winners as (key << 32) | ~index, unique per query, into win[q][0..m) (sel_collect).  Sliced:
//            per-slice counts (k_lk_count), each slice's offset from the counts of the slices before it (k_lk_write).
//   sort     descending on that 64-bit value = score descending, ties ascending index.  m <= kLkSortMax: one
//            workgroup per query sorts in LDS and gathers; above: tiles of kLkTile sorted in LDS, then merge
//            passes that place each entry by its rank in the partner run (k_lk_merge), the last one gathering.
//   gather   out_idx[q][i] = index, out_score[q][i] = row[index] (bit for bit), -1 / NaN for i >= m.
// After the kernels: the batch driver (topk_batches) and the entry points of both exact paths, this one and k_select's.
// ====================================================================================
namespace anirec {

constexpr int kLkSortMax = kLdsSortMax;  // one-workgroup sort (lds_sort_desc): 20480 x 8 B of LDS
constexpr int kLkTile = 16384;     // tile of the multi-workgroup sort (128 KiB of LDS)
constexpr size_t kLkHistBytes = (size_t)4 * kSelMaxBlocks * 256 * 4;  // [pass][query x slice][digit]
constexpr size_t kLkCntBytes = (size_t)kSelMaxBlocks * 2 * 4;         // [query x slice][gt, eq]

struct LkArgs {
  SelectArgs s;             // scores [nq][ld], masks, k, nq (this batch), slices; s.src_idx == nullptr
  unsigned long long *win;  // [nq][kcap] winners (key << 32) | ~index
  unsigned long long *win2; // [nq][kcap] second buffer of the merge passes
  size_t kcap;              // min(k, n): the most winners a query can have
  uint4 *st;                // [4][nq] state after each select pass: prefix, want, m, short
  uint32_t *hist;           // [4][nq * slices][256] digit histograms of the sliced select
  uint32_t *cnt;            // [nq * slices][2] winners above / at the threshold per slice
};

// many queries: one workgroup per query runs the whole select and collects its winners
__global__ __launch_bounds__(kSelThreads) void k_lk_select_row(LkArgs a) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sh[3];
  __shared__ uint32_t wsum[kSelThreads / 64];
  const int q = blockIdx.x;
  const SelectArgs &s = a.s;
  const float *row = s.scores + (size_t)q * s.ld;
  const int self = s.self ? s.self[q] : -1;
  uint4 st = make_uint4(0u, (uint32_t)s.k, (uint32_t)s.k, 0u);
  for (int pass = 0; pass < 4 && !st.w; ++pass) {
    sel_hist(s, row, q, self, 0, s.n, st.x, sel_pmask(pass), 24 - 8 * pass, hist);
    sel_digit(hist, st.x, st.y, 24 - 8 * pass, sh);
    st = sel_advance(st, sh);
    __syncthreads();
  }
  if (threadIdx.x == 0) a.st[3 * s.nq + q] = st;
  sel_collect(s, row, q, self, 0, s.n, st.w ? 0u : st.x, st.w ? 0xFFFFFFFFu : st.y, st.w != 0, 0, 0,
             a.win + (size_t)q * a.kcap, (uint32_t)a.kcap, wsum);
}

// Sliced select: the state after pass p - 1 of the workgroup's query, from the state after pass p - 2 and the slice
// histograms of pass p - 1.  Every workgroup of the query computes the same; slice 0 stores it for later launches.
__device__ uint4 lk_state(const LkArgs &a, int q, int slice, int pass, uint32_t *hist, uint32_t *sh) {
  const SelectArgs &s = a.s;
  const uint4 prev = pass >= 2 ? a.st[(size_t)(pass - 2) * s.nq + q] : make_uint4(0u, (uint32_t)s.k, (uint32_t)s.k, 0u);
  uint4 st = prev;
  if (!prev.w) {
    const uint32_t *h = a.hist + ((size_t)(pass - 1) * s.nq + q) * s.slices * 256;
    uint32_t sum = 0;
    for (int b = 0; b < s.slices; ++b) sum += h[(size_t)b * 256 + threadIdx.x];
    hist[threadIdx.x] = sum;
    __syncthreads();
    sel_digit(hist, prev.x, prev.y, 24 - 8 * (pass - 1), sh);
    st = sel_advance(prev, sh);
    __syncthreads();
  }
  if (slice == 0 && threadIdx.x == 0) a.st[(size_t)(pass - 1) * s.nq + q] = st;
  return st;
}

template <int kPass>
__global__ __launch_bounds__(kSelThreads) void k_lk_hist(LkArgs a) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sh[3];
  const SelectArgs &s = a.s;
  const int q = blockIdx.x / s.slices, slice = blockIdx.x % s.slices;
  const int j_lo = slice * s.slice_len, j_hi = min(s.n, j_lo + s.slice_len);
  const float *row = s.scores + (size_t)q * s.ld;
  const int self = s.self ? s.self[q] : -1;
  uint4 st = make_uint4(0u, (uint32_t)s.k, (uint32_t)s.k, 0u);
  if constexpr (kPass > 0) st = lk_state(a, q, slice, kPass, hist, sh);
  if (st.w) return;  // short row: every candidate wins, nothing left to locate
  sel_hist(s, row, q, self, j_lo, j_hi, st.x, sel_pmask(kPass), 24 - 8 * kPass, hist);
  a.hist[((size_t)kPass * s.nq * s.slices + blockIdx.x) * 256 + threadIdx.x] = hist[threadIdx.x];
}

// final state (pass 3) and, per slice, the keys above the threshold and at it
__global__ __launch_bounds__(kSelThreads) void k_lk_count(LkArgs a) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sh[3];
  __shared__ uint32_t tot[2];
  const SelectArgs &s = a.s;
  const int q = blockIdx.x / s.slices, slice = blockIdx.x % s.slices;
  const int j_lo = slice * s.slice_len, j_hi = min(s.n, j_lo + s.slice_len);
  const float *row = s.scores + (size_t)q * s.ld;
  const int self = s.self ? s.self[q] : -1;
  const uint4 st = lk_state(a, q, slice, 4, hist, sh);
  const uint32_t T = st.w ? 0u : st.x;
  if (threadIdx.x < 2) tot[threadIdx.x] = 0;
  __syncthreads();
  uint32_t c_gt = 0, c_eq = 0;
  for (int j = j_lo + threadIdx.x; j < j_hi; j += kSelThreads) {
    const uint32_t key = cand_key(s, row, q, j, self);
    if (key == 0u) continue;
    if (st.w || key > T) ++c_gt;
    else if (key == T) ++c_eq;
  }
  if (c_gt) atomicAdd(&tot[0], c_gt);
  if (c_eq) atomicAdd(&tot[1], c_eq);
  __syncthreads();
  if (threadIdx.x < 2) a.cnt[(size_t)blockIdx.x * 2 + threadIdx.x] = tot[threadIdx.x];
}

// each slice writes its winners after those of the slices before it
__global__ __launch_bounds__(kSelThreads) void k_lk_write(LkArgs a) {
  __shared__ uint32_t wsum[kSelThreads / 64];
  const SelectArgs &s = a.s;
  const int q = blockIdx.x / s.slices, slice = blockIdx.x % s.slices;
  const int j_lo = slice * s.slice_len, j_hi = min(s.n, j_lo + s.slice_len);
  const float *row = s.scores + (size_t)q * s.ld;
  const int self = s.self ? s.self[q] : -1;
  const uint4 st = a.st[(size_t)3 * s.nq + q];
  const uint32_t need_eq = st.w ? 0xFFFFFFFFu : st.y;
  uint32_t n_out = 0, eq_taken = 0;
  for (int b = 0; b < slice; ++b) {
    const uint32_t *c = a.cnt + ((size_t)q * s.slices + b) * 2;
    const uint32_t room = need_eq == 0xFFFFFFFFu ? 0u : need_eq - eq_taken;
    const uint32_t use = c[1] < room ? c[1] : room;
    n_out += c[0] + use;
    eq_taken += use;
  }
  sel_collect(s, row, q, self, j_lo, j_hi, st.w ? 0u : st.x, need_eq, st.w != 0, n_out, eq_taken,
             a.win + (size_t)q * a.kcap, (uint32_t)a.kcap, wsum);
}

// out row q, position i: the winner v, or the -1 / NaN pad
__device__ __forceinline__ void lk_out(const LkArgs &a, int q, size_t i, unsigned long long v, bool valid) {
  const SelectArgs &s = a.s;
  const size_t o = (size_t)q * s.k + i;
  if (valid) {
    const uint32_t j = ~(uint32_t)(v & 0xFFFFFFFFull);
    s.out_idx[o] = (int32_t)j;
    s.out_score[o] = s.scores[(size_t)q * s.ld + j];
  } else {
    s.out_idx[o] = -1;
    s.out_score[o] = __uint_as_float(0x7FC00000u);
  }
}

// Sort in LDS, descending, of the winners [t * tile, min(m, (t + 1) * tile)) of query blockIdx.x / tiles: a bitonic
// network in its one-direction form (each merge starts by comparing mirrored pairs), so the entries past the count
// are virtual zeros that no comparator moves and are skipped.  gather: tiles == 1 and tile == kcap, write the
// output rows; else write the sorted tile back.
__global__ __launch_bounds__(1024) void k_lk_sort(LkArgs a, int tiles, int tile, int gather) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sw[];
  const int q = blockIdx.x / tiles, t = blockIdx.x % tiles;
  const uint32_t m = a.st[(size_t)3 * a.s.nq + q].z;
  const uint32_t lo = (uint32_t)t * (uint32_t)tile;
  const uint32_t cnt = m > lo ? min(m - lo, (uint32_t)tile) : 0u;
  unsigned long long *w = a.win + (size_t)q * a.kcap + lo;
  const int tid = threadIdx.x, nt = blockDim.x;
  for (uint32_t i = tid; i < cnt; i += nt) sw[i] = w[i];
  __syncthreads();
  lds_sort_desc(sw, cnt, tid, nt);
  if (gather) {
    for (size_t i = tid; i < (size_t)a.s.k; i += nt) lk_out(a, q, i, i < cnt ? sw[i] : 0ull, i < cnt);
  } else {
    for (uint32_t i = tid; i < cnt; i += nt) w[i] = sw[i];
  }
}

// One merge pass over sorted runs of length L: the entry at i of run r goes to the start of the pair of runs plus
// its rank in its own run plus the entries of run r ^ 1 above it (binary search; the values are unique).  dst ==
// nullptr: the last pass, which writes the output rows (and pads them to k).
__global__ __launch_bounds__(256) void k_lk_merge(LkArgs a, const unsigned long long *src, unsigned long long *dst,
                                                  uint32_t L) {
  const int q = blockIdx.y;
  const uint32_t m = a.st[(size_t)3 * a.s.nq + q].z;
  const unsigned long long *r = src + (size_t)q * a.kcap;
  const size_t lim = dst ? (size_t)m : (size_t)a.s.k;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < lim; i += (size_t)gridDim.x * 256) {
    if (i >= m) {
      lk_out(a, q, i, 0ull, false);
      continue;
    }
    const uint32_t ii = (uint32_t)i;
    const uint32_t rs = ii / L * L, ps = (ii / L ^ 1u) * L;
    const uint32_t pe = ps < m ? min(ps + L, m) : ps;
    const unsigned long long v = r[ii];
    uint32_t lo = ps, hi = pe;  // first position of the partner run whose value is below v
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (r[mid] > v) lo = mid + 1;
      else hi = mid;
    }
    const uint32_t o = (ii - rs) + (lo - ps) + min(rs, ps);
    if (dst) dst[(size_t)q * a.kcap + o] = v;
    else lk_out(a, q, o, v, true);
  }
}

// select + collect + sort + gather for the a.s.nq score rows of one batch
static int lk_run(LkArgs a, hipStream_t s) {
  SelectArgs &sa = a.s;
  sa.src_idx = nullptr;
  const int S = select_slices(sa.nq, sa.n);
  sa.slices = S;
  sa.slice_len = (sa.n + S - 1) / S;
  if (S == 1) {
    hipLaunchKernelGGL(k_lk_select_row, dim3(sa.nq), dim3(kSelThreads), 0, s, a);
  } else {
    const dim3 g(sa.nq * S);
    hipLaunchKernelGGL(k_lk_hist<0>, g, dim3(kSelThreads), 0, s, a);
    hipLaunchKernelGGL(k_lk_hist<1>, g, dim3(kSelThreads), 0, s, a);
    hipLaunchKernelGGL(k_lk_hist<2>, g, dim3(kSelThreads), 0, s, a);
    hipLaunchKernelGGL(k_lk_hist<3>, g, dim3(kSelThreads), 0, s, a);
    hipLaunchKernelGGL(k_lk_count, g, dim3(kSelThreads), 0, s, a);
    hipLaunchKernelGGL(k_lk_write, g, dim3(kSelThreads), 0, s, a);
  }
  ANIREC_HIP_CHECK(hipGetLastError());
  ANIREC_HIP_CHECK(hipFuncSetAttribute((const void *)k_lk_sort, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       kLkSortMax * 8));
  if (a.kcap <= (size_t)kLkSortMax) {
    uint32_t npad = 1;
    while (npad < a.kcap) npad <<= 1;
    const int nt = npad / 2 < 64 ? 64 : (npad / 2 > 1024 ? 1024 : (int)(npad / 2));
    hipLaunchKernelGGL(k_lk_sort, dim3(sa.nq), dim3(nt), a.kcap * 8, s, a, 1, (int)a.kcap, 1);
    return (int)hipGetLastError();
  }
  const int tiles = (int)((a.kcap + kLkTile - 1) / kLkTile);
  hipLaunchKernelGGL(k_lk_sort, dim3(sa.nq * tiles), dim3(1024), (size_t)kLkTile * 8, s, a, tiles, kLkTile, 0);
  unsigned long long *src = a.win, *dst = a.win2;
  for (size_t L = kLkTile; L < a.kcap; L *= 2) {
    const bool last = 2 * L >= a.kcap;
    const size_t lim = last ? (size_t)sa.k : a.kcap;
    size_t bx = (lim + 255) / 256;
    if (bx > 4096) bx = 4096;
    hipLaunchKernelGGL(k_lk_merge, dim3((unsigned)bx, sa.nq), dim3(256), 0, s, a, src, last ? nullptr : dst,
                       (uint32_t)L);
    unsigned long long *t = src;
    src = dst;
    dst = t;
  }
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------
// the batch driver of the four exact top-k entry points: score rows for a batch of queries, then a select from them
// ------------------------------------------------------------------------------------
// The workspace of a call after its head (self[nq] of a cosine call, Ah | Uh of a predict call), for either select
// kind: a fixed part, then per query of a batch what bytes() sizes and carve() hands out.
//   launch_select  slice winners (kSelTmpBytes) | score rows
//   lk_run         hist | cnt | per query: a state, the winners (two buffers when the multi-workgroup sort merges),
//                  a score row
struct TopkLayout {
  bool large;        // the select kind: lk_run, else launch_select
  size_t kcap;       // large: min(k, n), the most winners a query can have
  size_t fixed, per_query;

  // a call of nq queries in batches of at most `cap`, halved while a batch is above `limit` bytes
  size_t bytes(size_t nq, size_t cap, size_t limit = (size_t)4 << 30) const {
    size_t qb = nq < cap ? nq : cap;
    while (qb > 1 && qb * per_query > limit) qb >>= 1;
    return fixed + qb * per_query;
  }
  // a batch of qb queries out of `p` (256-aligned); returns its score rows
  float *carve(char *p, size_t qb, LkArgs &la, void *&sel_tmp) const {
    if (!large) {
      sel_tmp = p;
      return (float *)(p + fixed);
    }
    la.hist = (uint32_t *)p;
    la.cnt = (uint32_t *)(p + kLkHistBytes);
    la.st = (uint4 *)(p + fixed);
    la.kcap = kcap;
    la.win = (unsigned long long *)(la.st + 4 * qb);
    la.win2 = kcap > (size_t)kLkSortMax ? la.win + qb * kcap : la.win;
    return (float *)(la.win2 + qb * kcap);
  }
};
static TopkLayout select_layout(int32_t n) { return {false, 0, kSelTmpBytes, (size_t)n * 4}; }
static TopkLayout lk_layout(int32_t n, int32_t k) {
  const size_t kc = (size_t)(k < n ? k : n);
  return {true, kc, kLkHistBytes + kLkCntBytes,
          4 * sizeof(uint4) + kc * 8 * (kc > (size_t)kLkSortMax ? 2 : 1) + (size_t)n * 4};
}
static size_t self_bytes(int32_t nq) { return ((size_t)nq * 4 + 255) / 256 * 256; }

// where the score rows come from: query q of the call is row (qrows ? qrows[q] : q) of Q
struct ScoreSource {
  const float *Q, *W;     // cosine: Q = W = What; predict: Uh, Ah
  const int32_t *qrows;   // cosine: the call's queries
  int dim;
  int use_head;           // predict: act(c * hs + hb)
  float hs, hb;
  int32_t act;
};
// what a query may not return (SelectArgs): all optional
struct RowMasks {
  const int32_t *self;    // [nq]
  const uint8_t *keep;    // [n]
  const uint32_t *wbits;  // [nq][(n + 31) / 32]
};

// `ws`: the workspace after its head, at least L.fixed + L.per_query bytes (the entry point has checked)
static int topk_batches(const ScoreSource &src, const RowMasks &m, const TopkLayout &L, int n, int nq, int k,
                        int32_t *out_idx, float *out_score, char *ws, size_t ws_bytes, hipStream_t s) {
  size_t qb = (ws_bytes - L.fixed) / L.per_query;
  if (qb > (size_t)nq) qb = nq;
  LkArgs la = {};
  void *sel_tmp = nullptr;
  float *buf = L.carve(ws, qb, la, sel_tmp);
  const int wwords = (n + 31) / 32;
  for (size_t q0 = 0; q0 < (size_t)nq; q0 += qb) {
    const int cnt = (int)((size_t)nq - q0 < qb ? (size_t)nq - q0 : qb);
    ScoreArgs a;
    a.Q = src.qrows ? src.Q : src.Q + q0 * src.dim;
    a.qrows = src.qrows ? src.qrows + q0 : nullptr;
    a.nq = cnt;
    a.W = src.W;
    a.n = n;
    a.out = buf;
    a.ld = (size_t)n;
    a.use_head = src.use_head;
    a.hs = src.hs;
    a.hb = src.hb;
    int e = launch_scores(a, s, src.act, src.dim);
    if (e) return e;
    SelectArgs &sa = la.s;
    sa.scores = buf;
    sa.ld = (size_t)n;
    sa.n = n;
    sa.nq = cnt;
    sa.k = k;
    sa.self = m.self ? m.self + q0 : nullptr;
    sa.keep = m.keep;
    sa.wbits = m.wbits ? m.wbits + q0 * wwords : nullptr;
    sa.wwords = wwords;
    sa.out_idx = out_idx + q0 * k;
    sa.out_score = out_score + q0 * k;
    e = L.large ? lk_run(la, s) : launch_select(sa, sel_tmp, s);
    if (e) return e;
  }
  return ANIREC_OK;
}

// the cosine calls: self[nq] (256-aligned) at the head of the workspace
static int cosine_topk(const TopkLayout &L, const float *What, int32_t n, int32_t dim, const int32_t *queries,
                       int32_t nq, const uint8_t *keep, int32_t exclude_self, int32_t k, int32_t *out_idx,
                       float *out_score, void *workspace, size_t workspace_bytes, hipStream_t s) {
  const size_t head = self_bytes(nq);
  if (workspace_bytes < head + L.fixed + L.per_query) return ANIREC_EWORKSPACE;
  int32_t *self = (int32_t *)workspace;
  hipLaunchKernelGGL(k_fill_self, dim3((nq + 255) / 256), dim3(256), 0, s, queries, nq, self, exclude_self);
  ANIREC_HIP_CHECK(hipGetLastError());
  const ScoreSource src = {What, What, queries, dim, 0, 0.f, 0.f, ANIREC_ACT_SIGMOID};
  const RowMasks m = {self, keep, nullptr};
  return topk_batches(src, m, L, n, nq, k, out_idx, out_score, (char *)workspace + head, workspace_bytes - head, s);
}

// the predict calls: Ah | Uh at the head of the workspace
static int predict_topk(const TopkLayout &L, const float *U, const float *A, int32_t dim, int32_t n_anime,
                        const int32_t *users, int32_t n_users, const anirec_head *head, int32_t activation,
                        const uint32_t *watched, int32_t k, int32_t *out_idx, float *out_p, void *workspace,
                        size_t workspace_bytes, hipStream_t s) {
  const size_t nb = norm_bytes(n_anime, n_users, dim);
  if (workspace_bytes < nb + L.fixed + L.per_query) return ANIREC_EWORKSPACE;
  NormRows t;
  ANIREC_HIP_CHECK(normalise_tables(U, A, dim, n_anime, users, n_users, workspace, s, &t));
  ScoreSource src = {t.Uh, t.Ah, nullptr, dim, 1, 0.f, 0.f, activation};
  head_affine(head, &src.hs, &src.hb);
  const RowMasks m = {nullptr, nullptr, watched};
  return topk_batches(src, m, L, n_anime, n_users, k, out_idx, out_p, (char *)workspace + nb, workspace_bytes - nb, s);
}

}  // namespace anirec

extern "C" {

// Batches: 1024 queries for cosine, 4096 for predict; the score rows of a batch are capped at 4 GiB (not in
// anirec_predict_workspace_bytes, which never was).  The least an entry point takes is the head, the fixed part and
// one query: it then runs one query per batch.
size_t anirec_topk_workspace_bytes(int32_t n, int32_t nq) {
  if (n < 1 || nq < 1) return 0;
  return self_bytes(nq) + select_layout(n).bytes(nq, 1024);
}

size_t anirec_topk_large_workspace_bytes(int32_t n, int32_t nq, int32_t k) {
  if (n < 1 || nq < 1 || k < 1) return 0;
  return self_bytes(nq) + lk_layout(n, k).bytes(nq, 1024);
}

size_t anirec_predict_workspace_bytes(int32_t n_anime, int32_t n_users, int32_t topk) {
  return anirec_predict_workspace_bytes_w(n_anime, n_users, topk, ANIREC_DIM);
}

// predict_grid (topk == 0): the normalised tables alone
size_t anirec_predict_workspace_bytes_w(int32_t n_anime, int32_t n_users, int32_t topk, int32_t dim) {
  if (n_anime < 1 || n_users < 1 || !dim_ok(dim)) return 0;
  return norm_bytes(n_anime, n_users, dim) + (topk ? select_layout(n_anime).bytes(n_users, 4096, SIZE_MAX) : 0);
}

size_t anirec_predict_topk_large_workspace_bytes(int32_t n_anime, int32_t n_users, int32_t k) {
  return anirec_predict_topk_large_workspace_bytes_w(n_anime, n_users, k, ANIREC_DIM);
}

size_t anirec_predict_topk_large_workspace_bytes_w(int32_t n_anime, int32_t n_users, int32_t k, int32_t dim) {
  if (n_anime < 1 || n_users < 1 || k < 1 || !dim_ok(dim)) return 0;
  return norm_bytes(n_anime, n_users, dim) + lk_layout(n_anime, k).bytes(n_users, 4096);
}

int anirec_cosine_topk(const float *What, int32_t n, const int32_t *queries, int32_t nq,
                       const uint8_t *keep, int32_t exclude_self, int32_t k, int32_t *out_idx,
                       float *out_score, void *workspace, size_t workspace_bytes, void *stream) {
  return anirec_cosine_topk_w(What, n, ANIREC_DIM, queries, nq, keep, exclude_self, k, out_idx, out_score, workspace,
                              workspace_bytes, stream);
}

int anirec_cosine_topk_w(const float *What, int32_t n, int32_t dim, const int32_t *queries, int32_t nq,
                         const uint8_t *keep, int32_t exclude_self, int32_t k, int32_t *out_idx,
                         float *out_score, void *workspace, size_t workspace_bytes, void *stream) {
  if (!What || !queries || !out_idx || !out_score || !workspace || !dim_ok(dim)) return ANIREC_EINVAL;
  if (n < 1 || nq < 0 || k < 1 || k > ANIREC_MAX_TOPK) return ANIREC_EINVAL;
  if (nq == 0) return ANIREC_OK;
  return cosine_topk(select_layout(n), What, n, dim, queries, nq, keep, exclude_self, k, out_idx, out_score,
                     workspace, workspace_bytes, (hipStream_t)stream);
}

int anirec_cosine_topk_large(const float *What, int32_t n, const int32_t *queries, int32_t nq, const uint8_t *keep,
                             int32_t exclude_self, int32_t k, int32_t *out_idx, float *out_score, void *workspace,
                             size_t workspace_bytes, void *stream) {
  return anirec_cosine_topk_large_w(What, n, ANIREC_DIM, queries, nq, keep, exclude_self, k, out_idx, out_score,
                                    workspace, workspace_bytes, stream);
}

// (the any-k kernels whatever k is: the entry point chooses the select kind)
int anirec_cosine_topk_large_w(const float *What, int32_t n, int32_t dim, const int32_t *queries, int32_t nq,
                               const uint8_t *keep, int32_t exclude_self, int32_t k, int32_t *out_idx,
                               float *out_score, void *workspace, size_t workspace_bytes, void *stream) {
  if (!What || !queries || !out_idx || !out_score || !workspace || !dim_ok(dim)) return ANIREC_EINVAL;
  if (n < 1 || nq < 0 || k < 1) return ANIREC_EINVAL;
  if (nq == 0) return ANIREC_OK;
  return cosine_topk(lk_layout(n, k), What, n, dim, queries, nq, keep, exclude_self, k, out_idx, out_score, workspace,
                     workspace_bytes, (hipStream_t)stream);
}

int anirec_predict_topk(const float *U, const float *A, int32_t n_anime, const int32_t *users,
                        int32_t n_users, const anirec_head *head, const uint32_t *watched,
                        int32_t k, int32_t *out_idx, float *out_p, void *workspace,
                        size_t workspace_bytes, void *stream) {
  return anirec_predict_topk_act(U, A, n_anime, users, n_users, head, ANIREC_ACT_SIGMOID, watched, k, out_idx, out_p,
                                 workspace, workspace_bytes, stream);
}

int anirec_predict_topk_act(const float *U, const float *A, int32_t n_anime, const int32_t *users,
                            int32_t n_users, const anirec_head *head, int32_t activation,
                            const uint32_t *watched, int32_t k, int32_t *out_idx, float *out_p, void *workspace,
                            size_t workspace_bytes, void *stream) {
  return anirec_predict_topk_w(U, A, ANIREC_DIM, n_anime, users, n_users, head, activation, watched, k, out_idx, out_p,
                               workspace, workspace_bytes, stream);
}

int anirec_predict_topk_w(const float *U, const float *A, int32_t dim, int32_t n_anime, const int32_t *users,
                          int32_t n_users, const anirec_head *head, int32_t activation,
                          const uint32_t *watched, int32_t k, int32_t *out_idx, float *out_p, void *workspace,
                          size_t workspace_bytes, void *stream) {
  if (!U || !A || !users || !head || !out_idx || !out_p || !workspace || !act_ok(activation) || !dim_ok(dim))
    return ANIREC_EINVAL;
  if (n_anime < 1 || n_users < 0 || k < 1 || k > ANIREC_MAX_TOPK) return ANIREC_EINVAL;
  if (n_users == 0) return ANIREC_OK;
  return predict_topk(select_layout(n_anime), U, A, dim, n_anime, users, n_users, head, activation, watched, k,
                      out_idx, out_p, workspace, workspace_bytes, (hipStream_t)stream);
}

int anirec_predict_topk_large_act(const float *U, const float *A, int32_t n_anime, const int32_t *users,
                                  int32_t n_users, const anirec_head *head, int32_t activation,
                                  const uint32_t *watched, int32_t k, int32_t *out_idx, float *out_p, void *workspace,
                                  size_t workspace_bytes, void *stream) {
  return anirec_predict_topk_large_w(U, A, ANIREC_DIM, n_anime, users, n_users, head, activation, watched, k, out_idx,
                                     out_p, workspace, workspace_bytes, stream);
}

int anirec_predict_topk_large_w(const float *U, const float *A, int32_t dim, int32_t n_anime, const int32_t *users,
                                int32_t n_users, const anirec_head *head, int32_t activation,
                                const uint32_t *watched, int32_t k, int32_t *out_idx, float *out_p, void *workspace,
                                size_t workspace_bytes, void *stream) {
  if (!U || !A || !users || !head || !out_idx || !out_p || !workspace || !act_ok(activation) || !dim_ok(dim))
    return ANIREC_EINVAL;
  if (n_anime < 1 || n_users < 0 || k < 1) return ANIREC_EINVAL;
  if (n_users == 0) return ANIREC_OK;
  return predict_topk(lk_layout(n_anime, k), U, A, dim, n_anime, users, n_users, head, activation, watched, k,
                      out_idx, out_p, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"

// ====================================================================================
// rank of a target anime among a user's unwatched anime (anirec_predict_rank) and the watched-bit table of a
// rating list (anirec_seen_bits)
//
// rank[t] = how many eligible anime come before target t in the user's whole ranking (anirec_predict_topk_large_*):
// a count, so no rating row is written and nothing is sorted.  The ratings are the exact path's, bit for bit: rows
// through rownorm_body<1>, the k-ordered fma chain of scores_body, rating_from_cosine; the order is score_key's.
//   targets  one thread per target: its indices checked, p[t] by the chain, rank[t] = 0 (k_rank_targets)
//   count    a workgroup holds 64 targets' user rows in LDS (whole rows: pitch width + 4) and walks the 64-row
//            tiles of its slice of the anime table, scores_body's 4 x 4 register block per thread; the epilogue
//            compares each rating's key with the target's and counts.  The per-slice counts of a target meet in an
//            integer atomicAdd: any order gives the same sum (k_rank_count)
// ====================================================================================
namespace anirec {

struct RankArgs {
  const float *Uh;         // [n_users, dim] normalised rows of the call's users
  const float *Ah;         // [n_anime, dim] normalised
  int n_users, n_anime;
  const int32_t *trow;     // [n_targets] row of target t in the users list
  const int32_t *tanime;   // [n_targets] its anime
  int n_targets;
  const uint32_t *watched; // optional [n_users][wwords]: set bit = not eligible (the target's own bit is ignored)
  int wwords;
  float hs, hb;
  int act;
  int slices, slice_len;   // workgroup b counts targets [64 (b / slices), +64) over anime [(b % slices) slice_len, +slice_len)
  int32_t *rank;           // [n_targets]
  float *p;                // [n_targets]
  int32_t *err;
};

__device__ __forceinline__ bool rank_target_ok(const RankArgs &a, int row, int at) {
  return (uint32_t)row < (uint32_t)a.n_users && (uint32_t)at < (uint32_t)a.n_anime;
}

template <int kD>
__global__ __launch_bounds__(256) void k_rank_targets(RankArgs a) {
  constexpr int kRowV = kD / 4;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= a.n_targets) return;
  const int row = a.trow[t], at = a.tanime[t];
  if (!rank_target_ok(a, row, at)) {  // nothing is read through a bad index
    *a.err = 1;
    a.rank[t] = -1;
    a.p[t] = __uint_as_float(0x7FC00000u);
    return;
  }
  const float4 *q4 = reinterpret_cast<const float4 *>(a.Uh) + (size_t)row * kRowV;
  const float4 *w4 = reinterpret_cast<const float4 *>(a.Ah) + (size_t)at * kRowV;
  float s = 0.f;
#pragma unroll 8
  for (int k4 = 0; k4 < kRowV; ++k4) {
    const float4 x = w4[k4], y = q4[k4];
    s = __fmaf_rn(x.x, y.x, s);
    s = __fmaf_rn(x.y, y.y, s);
    s = __fmaf_rn(x.z, y.z, s);
    s = __fmaf_rn(x.w, y.w, s);
  }
  a.p[t] = rating_from_cosine<-1>(s, a.hs, a.hb, a.act);
  a.rank[t] = 0;
}

template <int kD>
__global__ __launch_bounds__(256) void k_rank_count(RankArgs a) {
  constexpr int kSV = ScoreGeom<kD>::kSV, kPitch = ScoreGeom<kD>::kPitch, kRowV = ScoreGeom<kD>::kRowV;
  constexpr int kQPitch = kD + 4;  // the targets' rows stay whole: staged once for every tile of the slice
  __shared__ __attribute__((aligned(16))) float Qs[kTile * kQPitch];
  __shared__ __attribute__((aligned(16))) float Ws[kTile * kPitch];
  const int tid = threadIdx.x;
  const int q0 = (blockIdx.x / a.slices) * kTile;
  const int j_lo = (blockIdx.x % a.slices) * a.slice_len;  // a multiple of 64: a tile's watched bits are two whole words
  const int j_hi = min(a.n_anime, j_lo + a.slice_len);
  const int tx = tid & 15, ty = tid >> 4;  // rows tx+16r, targets ty+16q
  int at[4], wrow[4], cnt[4];              // at < 0: no target
  uint32_t kt[4];
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) {
    const int t = q0 + ty + 16 * qq;
    at[qq] = -1;
    wrow[qq] = 0;
    kt[qq] = 0u;
    cnt[qq] = 0;
    if (t < a.n_targets) {
      const int row = a.trow[t], x = a.tanime[t];
      if (rank_target_ok(a, row, x)) {
        at[qq] = x;
        wrow[qq] = row;
        kt[qq] = score_key(a.p[t]);
      }
    }
  }
  for (int e = tid; e < kTile * kRowV; e += 256) {
    const int r = e / kRowV, cidx = e % kRowV;
    float4 qv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q0 + r < a.n_targets) {
      const int row = a.trow[q0 + r];
      if ((uint32_t)row < (uint32_t)a.n_users) qv = reinterpret_cast<const float4 *>(a.Uh)[(size_t)row * kRowV + cidx];
    }
    *reinterpret_cast<float4 *>(&Qs[r * kQPitch + cidx * 4]) = qv;
  }
  for (int j0 = j_lo; j0 < j_hi; j0 += kTile) {
    float acc[4][4];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[qq][r] = 0.f;
#pragma unroll
    for (int k0 = 0; k0 < kRowV; k0 += kSV) {  // (one pass up to 128)
      __syncthreads();                         // the previous tile / slice has been read
      for (int e = tid; e < kTile * kSV; e += 256) {
        const int r = e / kSV, cidx = e % kSV;
        float4 wv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j0 + r < a.n_anime) wv = reinterpret_cast<const float4 *>(a.Ah)[(size_t)(j0 + r) * kRowV + k0 + cidx];
        *reinterpret_cast<float4 *>(&Ws[r * kPitch + cidx * 4]) = wv;
      }
      __syncthreads();
#pragma unroll 4
      for (int k4 = 0; k4 < kSV; ++k4) {
        float4 qv[4], wv[4];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
          qv[qq] = *reinterpret_cast<const float4 *>(&Qs[(ty + 16 * qq) * kQPitch + (k0 + k4) * 4]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          wv[r] = *reinterpret_cast<const float4 *>(&Ws[(tx + 16 * r) * kPitch + k4 * 4]);
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float s = acc[qq][r];
            s = __fmaf_rn(wv[r].x, qv[qq].x, s);
            s = __fmaf_rn(wv[r].y, qv[qq].y, s);
            s = __fmaf_rn(wv[r].z, qv[qq].z, s);
            s = __fmaf_rn(wv[r].w, qv[qq].w, s);
            acc[qq][r] = s;
          }
      }
    }
    const int w0 = j0 >> 5;
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      if (at[qq] < 0) continue;
      uint32_t wb[2] = {0u, 0u};  // watched bits of anime j0 .. j0 + 63
      if (a.watched) {
        const uint32_t *wr = a.watched + (size_t)wrow[qq] * a.wwords;
        wb[0] = wr[w0];
        if (w0 + 1 < a.wwords) wb[1] = wr[w0 + 1];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = j0 + tx + 16 * r;
        if (j >= a.n_anime || j == at[qq]) continue;
        if ((wb[r >> 1] >> (tx + 16 * (r & 1))) & 1u) continue;
        const uint32_t key = score_key(rating_from_cosine<-1>(acc[qq][r], a.hs, a.hb, a.act));
        cnt[qq] += (key > kt[qq] || (key == kt[qq] && j < at[qq])) ? 1 : 0;
      }
    }
  }
#pragma unroll
  for (int qq = 0; qq < 4; ++qq) {
    int c = cnt[qq];  // the 16 lanes tx = 0..15 of a target are neighbours in the wave
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) c += __shfl_xor(c, o, 16);
    if (tx == 0 && at[qq] >= 0 && c) atomicAdd(&a.rank[q0 + ty + 16 * qq], c);
  }
}

__global__ __launch_bounds__(256) void k_seen_bits(const int32_t *__restrict__ user_idx,
                                                   const int32_t *__restrict__ anime_idx, long long n, int n_users,
                                                   int n_anime, int wwords, uint32_t *__restrict__ bits,
                                                   int32_t *__restrict__ err) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int u = user_idx[i], x = anime_idx[i];
  if ((uint32_t)u >= (uint32_t)n_users || (uint32_t)x >= (uint32_t)n_anime) {
    *err = 1;
    return;
  }
  atomicOr(&bits[(size_t)u * wwords + (x >> 5)], 1u << (x & 31));
}

// slices of the anime table per block of 64 targets: enough workgroups to fill the chip when the targets are few
constexpr int kRankBlocks = 1024;

// ------------------------------------------------------------------------------------
// the same rank under ONE score vector shared by all users (anirec_score_rank): the popularity baseline.  Nothing is
// multiplied, so a target costs n_anime compares: one wave per target, four targets per workgroup.  Lane l walks anime
// l, l + 64, ...: score[j] is a coalesced load of a vector that stays in cache, the 64 anime of a step lie in two
// watched words of the target's row (each lane reads its own: two distinct addresses per load), the count stays in a
// register and the wave adds up once.  No workspace, no atomics, no LDS.
// ------------------------------------------------------------------------------------
// ld: floats between the score rows of two users (anirec_rows_rank); 0 = the one shared vector.
__global__ __launch_bounds__(256) void k_score_rank(const float *__restrict__ score_rows, size_t ld, int n_anime,
                                                    const uint32_t *__restrict__ watched, int n_users,
                                                    const int32_t *__restrict__ trow, const int32_t *__restrict__ tanime,
                                                    int n_targets, int32_t *__restrict__ rank, int32_t *__restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);  // the same for the whole wave
  if (t >= n_targets) return;
  const int row = trow[t], at = tanime[t];
  if ((uint32_t)row >= (uint32_t)n_users || (uint32_t)at >= (uint32_t)n_anime) {  // nothing is read through a bad index
    if (lane == 0) {
      *err = 1;
      rank[t] = -1;
    }
    return;
  }
  const float *__restrict__ score = score_rows + (size_t)row * ld;
  const uint32_t kt = score_key(score[at]);
  const uint32_t *wr = watched ? watched + (size_t)row * (size_t)((n_anime + 31) >> 5) : nullptr;
  int cnt = 0;
#pragma unroll 4
  for (int j = lane; j < n_anime; j += 64) {  // j < n_anime: word j >> 5 is inside the row, bits past n_anime are never looked at
    const uint32_t key = score_key(score[j]);
    const uint32_t seen = wr ? (wr[j >> 5] >> (j & 31)) & 1u : 0u;
    const bool before = key > kt || (key == kt && j < at);
    cnt += (before && !seen && j != at) ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) rank[t] = cnt;
}

}  // namespace anirec

extern "C" {

size_t anirec_predict_rank_workspace_bytes(int32_t n_anime, int32_t n_users, int32_t n_targets, int32_t dim) {
  if (n_anime < 1 || n_users < 1 || n_targets < 0 || !dim_ok(dim)) return 0;
  return norm_bytes(n_anime, n_users, dim);
}

int anirec_predict_rank(const float *U, const float *A, int32_t dim, int32_t n_anime, const int32_t *users,
                        int32_t n_users, const anirec_head *head, int32_t activation, const uint32_t *watched,
                        const int32_t *target_row, const int32_t *target_anime, int32_t n_targets, int32_t *out_rank,
                        float *out_p, int32_t *err_flag, void *workspace, size_t workspace_bytes, void *stream) {
  if (!dim_ok(dim) || !act_ok(activation) || n_anime < 1 || n_users < 0 || n_targets < 0) return ANIREC_EINVAL;
  if (n_targets == 0 || n_users == 0) return ANIREC_OK;
  if (!U || !A || !users || !head || !target_row || !target_anime || !out_rank || !out_p || !err_flag || !workspace)
    return ANIREC_EINVAL;
  if (workspace_bytes < norm_bytes(n_anime, n_users, dim)) return ANIREC_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  NormRows t;
  ANIREC_HIP_CHECK(normalise_tables(U, A, dim, n_anime, users, n_users, workspace, s, &t));
  RankArgs a;
  a.Uh = t.Uh;
  a.Ah = t.Ah;
  a.n_users = n_users;
  a.n_anime = n_anime;
  a.trow = target_row;
  a.tanime = target_anime;
  a.n_targets = n_targets;
  a.watched = watched;
  a.wwords = (n_anime + 31) / 32;
  head_affine(head, &a.hs, &a.hb);
  a.act = activation;
  a.rank = out_rank;
  a.p = out_p;
  a.err = err_flag;
  const int tblocks = (n_targets + kTile - 1) / kTile, tiles = (n_anime + kTile - 1) / kTile;
  int S = tblocks < kRankBlocks ? kRankBlocks / tblocks : 1;
  if (S > tiles) S = tiles;
  a.slice_len = (tiles + S - 1) / S * kTile;
  a.slices = (n_anime + a.slice_len - 1) / a.slice_len;
  const dim3 g0((n_targets + 255) / 256), g1((unsigned)tblocks * (unsigned)a.slices);
  with_width(dim, [&](auto kd) {
    constexpr int kD = decltype(kd)::value;
    hipLaunchKernelGGL(k_rank_targets<kD>, g0, dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_rank_count<kD>, g1, dim3(256), 0, s, a);
  });
  return (int)hipGetLastError();
}

int anirec_seen_bits(const int32_t *user_idx, const int32_t *anime_idx, int64_t n, int32_t n_users, int32_t n_anime,
                     uint32_t *bits, int32_t *err_flag, void *stream) {
  if (n < 0 || n_users < 0 || n_anime < 1 || !err_flag || (n > 0 && (!user_idx || !anime_idx))) return ANIREC_EINVAL;
  if (n_users > 0 && !bits) return ANIREC_EINVAL;
  if (n >= ((int64_t)1 << 39)) return ANIREC_EINVAL;  // one thread per rating, 256 per workgroup
  hipStream_t s = (hipStream_t)stream;
  const int wwords = (n_anime + 31) / 32;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  if (n_users > 0) ANIREC_HIP_CHECK(hipMemsetAsync(bits, 0, (size_t)n_users * wwords * 4, s));
  if (n == 0) return ANIREC_OK;
  hipLaunchKernelGGL(k_seen_bits, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, user_idx, anime_idx, (long long)n,
                     n_users, n_anime, wwords, bits, err_flag);
  return (int)hipGetLastError();
}

int anirec_score_rank(const float *score, int32_t n_anime, const uint32_t *watched, int32_t n_users,
                      const int32_t *target_row, const int32_t *target_anime, int32_t n_targets, int32_t *out_rank,
                      int32_t *err_flag, void *stream) {
  if (n_anime < 1 || n_users < 0 || n_targets < 0) return ANIREC_EINVAL;
  if (n_targets == 0) return ANIREC_OK;
  if (!score || !target_row || !target_anime || !out_rank || !err_flag) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  hipLaunchKernelGGL(k_score_rank, dim3(((unsigned)n_targets + 3u) / 4u), dim3(256), 0, s, score, (size_t)0, n_anime,
                     watched, n_users, target_row, target_anime, n_targets, out_rank, err_flag);
  return (int)hipGetLastError();
}

int anirec_rows_rank(const float *scores, int64_t ld, int32_t n_anime, const uint32_t *watched, int32_t n_users,
                     const int32_t *target_row, const int32_t *target_anime, int32_t n_targets, int32_t *out_rank,
                     int32_t *err_flag, void *stream) {
  if (n_anime < 1 || n_users < 0 || n_targets < 0 || (ld != 0 && ld < n_anime)) return ANIREC_EINVAL;
  if (n_targets == 0) return ANIREC_OK;
  if (!scores || !target_row || !target_anime || !out_rank || !err_flag) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  hipLaunchKernelGGL(k_score_rank, dim3(((unsigned)n_targets + 3u) / 4u), dim3(256), 0, s, scores, (size_t)ld, n_anime,
                     watched, n_users, target_row, target_anime, n_targets, out_rank, err_flag);
  return (int)hipGetLastError();
}

}  // extern "C"

// ====================================================================================
// group recommendations (anirec_group_topk): a second feeder of the exact select
//
// One score row and one mask row per GROUP instead of per user, from one launch; the select (launch_select / lk_run)
// then runs on them as on the rows of launch_scores.  The member ratings are predict_grid's, bit for bit: rows through
// rownorm_body<1>, the k-ordered fma chain of scores_body in its 64 x 64 tile / 4 x 4 register block / pitch-132
// geometry, rating_from_cosine.  No [members, n_anime] matrix exists.
//   scores   a group holds m_pad = next_pow2(max_members) of a tile's 64 slots (64 / m_pad whole groups a tile: no
//            group straddles one; slots past a group's count stage zero rows and are ignored).  After the chain the
//            64 x 64 ratings go to LDS over the staging tiles, and one wave per (group of the tile, 64 anime) folds
//            them in member order, ballots the floor test, ORs the members' watched words and the group's exclude
//            words (a tile starts at a multiple of 64: two whole words) and stores the 64 aggregates and the two mask
//            words.  A group with a bad offsets pair or member row raises *err and gets an all-ones mask, as does an
//            empty one (no error): the select pads its rows with -1 / NaN (k_group_scores)
//   select   launch_select (k <= ANIREC_MAX_TOPK) or lk_run on the batch's rows, wbits = the mask rows
//   members  out_member_p[e][s] = the rating of member e for pick s of its group, one chain per thread
//            (k_group_member_p)
// No atomics, no host synchronisation.
// ====================================================================================
namespace anirec {

struct GroupArgs {
  const float *Uh;            // [n_users, dim] normalised rows of the call's users
  const float *Ah;            // [n_anime, dim] normalised
  int n_users, n_anime;
  const int32_t *offsets;     // [n_groups + 1]
  const int32_t *member_row;  // [n_members] positions in the users list
  int n_members, max_members;
  int m_shift;                // m_pad = 1 << m_shift slots per group
  int g0, ng;                 // the batch: groups [g0, g0 + ng) of the call
  const uint32_t *watched;    // optional [n_users][wwords]
  const uint32_t *exclude;    // optional [n_groups][wwords]
  int wwords;
  int mode;
  float floor, hs, hb;
  int act;
  float *score;               // [ng][n_anime] aggregate of each group of the batch
  uint32_t *mask;             // [ng][wwords] set bit = not a candidate
  int32_t *err;
};

__device__ __forceinline__ bool group_span_ok(const GroupArgs &a, int lo, int hi) {
  return lo >= 0 && hi >= lo && hi <= a.n_members && hi - lo <= a.max_members;
}

constexpr int kGroupPitch = kTile + 16;  // ratings tile in LDS: the four rows ty = 0..3 of a wave's store fall on distinct banks

template <int kD>
__global__ __launch_bounds__(256) void k_group_scores(GroupArgs a) {
  constexpr int kSV = ScoreGeom<kD>::kSV, kPitch = ScoreGeom<kD>::kPitch, kRowV = ScoreGeom<kD>::kRowV;
  constexpr int kStage = 2 * kTile * kPitch, kFold = kTile * kGroupPitch;
  __shared__ __attribute__((aligned(16))) float buf[kStage > kFold ? kStage : kFold];
  __shared__ int32_t slot_row[kTile];  // row (in the users list) of the member in each slot, -1: none
  __shared__ int32_t grp_cnt[kTile];   // per group of the tile: its count, -1: bad, -2: past the batch
  float *Qs = buf, *Ws = buf + kTile * kPitch, *P = buf;
  const int tid = threadIdx.x;
  const int j0 = blockIdx.x * kTile;
  const int m_pad = 1 << a.m_shift, gpt = kTile >> a.m_shift;
  const int gt0 = blockIdx.y * gpt;  // first group of the tile, within the batch
  if (tid < kTile) {                 // wave 0: slot tid = member tid % m_pad of group tid / m_pad
    const int gl = tid >> a.m_shift, i = tid & (m_pad - 1);
    const int g = gt0 + gl;
    int row = -1, cnt = -2;
    bool bad = false;
    if (g < a.ng) {
      const int lo = a.offsets[a.g0 + g], hi = a.offsets[a.g0 + g + 1];
      if (!group_span_ok(a, lo, hi)) {  // nothing is read through a bad value
        bad = true;
      } else {
        cnt = hi - lo;
        if (i < cnt) {
          row = a.member_row[lo + i];
          if ((uint32_t)row >= (uint32_t)a.n_users) {
            bad = true;
            row = -1;
          }
        }
      }
    }
    const unsigned long long span = (m_pad == 64 ? ~0ull : (1ull << m_pad) - 1ull) << (gl * m_pad);
    const bool gbad = (__ballot(bad) & span) != 0ull;  // a group's slots are neighbours in the wave
    slot_row[tid] = gbad ? -1 : row;
    if (i == 0) {
      grp_cnt[gl] = g < a.ng ? (gbad ? -1 : cnt) : -2;
      if (gbad && blockIdx.x == 0) *a.err = 1;
    }
  }
  __syncthreads();
  const int tx = tid & 15, ty = tid >> 4;  // anime tx+16r, slots ty+16q
  float acc[4][4];
#pragma unroll
  for (int qq = 0; qq < 4; ++qq)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[qq][r] = 0.f;
#pragma unroll
  for (int k0 = 0; k0 < kRowV; k0 += kSV) {  // (one pass up to 128)
    if (k0) __syncthreads();                 // the previous slice has been read
    for (int e = tid; e < kTile * kSV; e += 256) {
      const int r = e / kSV, cidx = e % kSV;
      float4 qv = make_float4(0.f, 0.f, 0.f, 0.f), wv = qv;
      const int src = slot_row[r];
      if (src >= 0) qv = reinterpret_cast<const float4 *>(a.Uh)[(size_t)src * kRowV + k0 + cidx];
      if (j0 + r < a.n_anime) wv = reinterpret_cast<const float4 *>(a.Ah)[(size_t)(j0 + r) * kRowV + k0 + cidx];
      *reinterpret_cast<float4 *>(&Qs[r * kPitch + cidx * 4]) = qv;
      *reinterpret_cast<float4 *>(&Ws[r * kPitch + cidx * 4]) = wv;
    }
    __syncthreads();
#pragma unroll 4
    for (int k4 = 0; k4 < kSV; ++k4) {
      float4 qv[4], wv[4];
#pragma unroll
      for (int qq = 0; qq < 4; ++qq)
        qv[qq] = *reinterpret_cast<const float4 *>(&Qs[(ty + 16 * qq) * kPitch + k4 * 4]);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        wv[r] = *reinterpret_cast<const float4 *>(&Ws[(tx + 16 * r) * kPitch + k4 * 4]);
#pragma unroll
      for (int qq = 0; qq < 4; ++qq)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float s = acc[qq][r];
          s = __fmaf_rn(wv[r].x, qv[qq].x, s);
          s = __fmaf_rn(wv[r].y, qv[qq].y, s);
          s = __fmaf_rn(wv[r].z, qv[qq].z, s);
          s = __fmaf_rn(wv[r].w, qv[qq].w, s);
          acc[qq][r] = s;
        }
    }
  }
  __syncthreads();  // the staging tiles have been read: the ratings take their place
#pragma unroll
  for (int qq = 0; qq < 4; ++qq)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      P[(ty + 16 * qq) * kGroupPitch + tx + 16 * r] = rating_from_cosine<-1>(acc[qq][r], a.hs, a.hb, a.act);
  __syncthreads();
  // one wave per group of the tile; lane = anime j0 + lane
  const int lane = tid & 63, w0 = j0 >> 5;
  const int j = j0 + lane;
  for (int gl = tid >> 6; gl < gpt; gl += 4) {
    const int cnt = grp_cnt[gl];
    if (cnt == -2) break;  // past the batch, and so is every later group of the tile
    const int g = gt0 + gl;
    uint32_t m_lo = 0xFFFFFFFFu, m_hi = 0xFFFFFFFFu;  // bad or empty: no candidates
    if (cnt > 0) {
#pragma clang fp contract(off)
      const float *pg = P + (gl << a.m_shift) * kGroupPitch + lane;
      float p = pg[0], s = p;
      bool below = p < a.floor;  // false for a NaN rating
      for (int i = 1; i < cnt; ++i) {
        p = pg[i * kGroupPitch];
        below |= p < a.floor;
        if (a.mode == ANIREC_GROUP_MEAN) {
          s = s + p;
        } else if (p != p) {
          s = p;  // a NaN sticks
        } else if (s == s && (a.mode == ANIREC_GROUP_MIN ? p < s : p > s)) {
          s = p;  // strict: of +-0 the earlier member stays
        }
      }
      if (a.mode == ANIREC_GROUP_MEAN) s = s / (float)cnt;
      const unsigned long long b = __ballot(below);
      m_lo = (uint32_t)b;
      m_hi = (uint32_t)(b >> 32);
      uint32_t x_lo = 0u, x_hi = 0u;  // lane i: the words of member i; lane 0 also the group's exclude words
      if (a.watched && lane < cnt) {
        const uint32_t *wr = a.watched + (size_t)slot_row[(gl << a.m_shift) + lane] * a.wwords;
        x_lo = wr[w0];
        if (w0 + 1 < a.wwords) x_hi = wr[w0 + 1];
      }
      if (a.exclude && lane == 0) {
        const uint32_t *xr = a.exclude + (size_t)(a.g0 + g) * a.wwords;
        x_lo |= xr[w0];
        if (w0 + 1 < a.wwords) x_hi |= xr[w0 + 1];
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        x_lo |= __shfl_xor(x_lo, o, 64);
        x_hi |= __shfl_xor(x_hi, o, 64);
      }
      m_lo |= x_lo;
      m_hi |= x_hi;
      if (j < a.n_anime) a.score[(size_t)g * a.n_anime + j] = s;
    }
    if (lane == 0) {
      uint32_t *mr = a.mask + (size_t)g * a.wwords;
      mr[w0] = m_lo;
      if (w0 + 1 < a.wwords) mr[w0 + 1] = m_hi;  // (the last tile of a table with n_anime % 64 in 1..32 has one word)
    }
  }
}

// out_member_p[e][s] = rating of member e for pick s of its group g = blockIdx.x; rows no valid group covers keep the
// NaN the entry point filled them with
template <int kD>
__global__ __launch_bounds__(256) void k_group_member_p(GroupArgs a, const int32_t *__restrict__ out_idx, int k,
                                                        float *__restrict__ out_member_p) {
  constexpr int kRowV = kD / 4;
  const int g = blockIdx.x;
  const int lo = a.offsets[g], hi = a.offsets[g + 1];
  if (!group_span_ok(a, lo, hi)) return;
  const size_t items = (size_t)(hi - lo) * k;
  for (size_t t = (size_t)blockIdx.y * 256 + threadIdx.x; t < items; t += (size_t)gridDim.y * 256) {
    const int e = lo + (int)(t / k), sl = (int)(t % k);
    const int jj = out_idx[(size_t)g * k + sl], row = a.member_row[e];
    float v = __uint_as_float(0x7FC00000u);
    if ((uint32_t)jj < (uint32_t)a.n_anime && (uint32_t)row < (uint32_t)a.n_users) {
      const float4 *q4 = reinterpret_cast<const float4 *>(a.Uh) + (size_t)row * kRowV;
      const float4 *w4 = reinterpret_cast<const float4 *>(a.Ah) + (size_t)jj * kRowV;
      float s = 0.f;
#pragma unroll 8
      for (int k4 = 0; k4 < kRowV; ++k4) {
        const float4 x = w4[k4], y = q4[k4];
        s = __fmaf_rn(x.x, y.x, s);
        s = __fmaf_rn(x.y, y.y, s);
        s = __fmaf_rn(x.z, y.z, s);
        s = __fmaf_rn(x.w, y.w, s);
      }
      v = rating_from_cosine<-1>(s, a.hs, a.hb, a.act);
    }
    out_member_p[(size_t)e * k + sl] = v;
  }
}

// the select's share of a group (either kind) and its mask row, which lies after the batch's score rows
static TopkLayout group_layout(int32_t n, int32_t k) {
  TopkLayout L = k <= ANIREC_MAX_TOPK ? select_layout(n) : lk_layout(n, k);
  L.per_query += (size_t)((n + 31) / 32) * 4;
  return L;
}

static bool group_shape_ok(int32_t n_anime, int32_t n_users, int32_t n_groups, int32_t k, int32_t dim) {
  return dim_ok(dim) && n_anime >= 1 && n_users >= 0 && n_groups >= 0 && k >= 1;
}

}  // namespace anirec

extern "C" {

size_t anirec_group_topk_workspace_bytes(int32_t n_anime, int32_t n_users, int32_t n_groups, int32_t k, int32_t dim) {
  if (!group_shape_ok(n_anime, n_users, n_groups, k, dim)) return 0;
  return norm_bytes(n_anime, n_users, dim) + group_layout(n_anime, k).bytes(n_groups < 1 ? 1 : n_groups, 4096);
}

int anirec_group_topk(const float *U, const float *A, int32_t dim, int32_t n_anime, const int32_t *users,
                      int32_t n_users, const anirec_head *head, int32_t activation, const uint32_t *watched,
                      const int32_t *group_offsets, const int32_t *member_row, int32_t n_groups, int32_t n_members,
                      int32_t max_members, const uint32_t *exclude, int32_t mode, float floor, int32_t k,
                      int32_t *out_idx, float *out_score, float *out_member_p, int32_t *err_flag, void *workspace,
                      size_t workspace_bytes, void *stream) {
  if (!group_shape_ok(n_anime, n_users, n_groups, k, dim) || !act_ok(activation) || n_members < 0 ||
      mode < ANIREC_GROUP_MEAN || mode > ANIREC_GROUP_MAX || floor != floor || max_members < 1 ||
      max_members > ANIREC_GROUP_MAX_MEMBERS)
    return ANIREC_EINVAL;
  if (n_groups == 0) return ANIREC_OK;
  if (!U || !A || !head || !group_offsets || !out_idx || !out_score || !err_flag || !workspace ||
      (n_users > 0 && !users) || (n_members > 0 && !member_row))
    return ANIREC_EINVAL;
  const size_t nb = norm_bytes(n_anime, n_users, dim);
  const TopkLayout L = group_layout(n_anime, k);
  if (workspace_bytes < nb + L.fixed + L.per_query) return ANIREC_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  if (out_member_p && n_members > 0)
    ANIREC_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)out_member_p, 0x7FC00000, (size_t)n_members * k, s));
  NormRows t;
  if (n_users > 0) {
    ANIREC_HIP_CHECK(normalise_tables(U, A, dim, n_anime, users, n_users, workspace, s, &t));
  } else {  // no rows to read: every member is out of range
    t.Ah = (float *)workspace;
    t.Uh = t.Ah + (size_t)n_anime * dim;
    launch_rownorm<1>(A, nullptr, n_anime, t.Ah, dim, s);
    ANIREC_HIP_CHECK(hipGetLastError());
  }
  GroupArgs a;
  a.Uh = t.Uh;
  a.Ah = t.Ah;
  a.n_users = n_users;
  a.n_anime = n_anime;
  a.offsets = group_offsets;
  a.member_row = member_row;
  a.n_members = n_members;
  a.max_members = max_members;
  a.m_shift = 0;
  while ((1 << a.m_shift) < max_members) ++a.m_shift;
  a.watched = watched;
  a.exclude = exclude;
  a.wwords = (n_anime + 31) / 32;
  a.mode = mode;
  a.floor = floor;
  head_affine(head, &a.hs, &a.hb);
  a.act = activation;
  a.err = err_flag;
  char *ws = (char *)workspace + nb;
  size_t gb = (workspace_bytes - nb - L.fixed) / L.per_query;
  if (gb > (size_t)n_groups) gb = n_groups;
  LkArgs la = {};
  void *sel_tmp = nullptr;
  a.score = L.carve(ws, gb, la, sel_tmp);
  a.mask = (uint32_t *)(a.score + gb * (size_t)n_anime);
  const int gpt = kTile >> a.m_shift;
  for (size_t g0 = 0; g0 < (size_t)n_groups; g0 += gb) {
    a.g0 = (int)g0;
    a.ng = (int)((size_t)n_groups - g0 < gb ? (size_t)n_groups - g0 : gb);
    const dim3 grid((n_anime + kTile - 1) / kTile, (a.ng + gpt - 1) / gpt);
    with_width(dim, [&](auto kd) {
      hipLaunchKernelGGL(k_group_scores<decltype(kd)::value>, grid, dim3(256), 0, s, a);
    });
    ANIREC_HIP_CHECK(hipGetLastError());
    SelectArgs &sa = la.s;
    sa.scores = a.score;
    sa.ld = (size_t)n_anime;
    sa.n = n_anime;
    sa.nq = a.ng;
    sa.k = k;
    sa.self = nullptr;
    sa.keep = nullptr;
    sa.wbits = a.mask;
    sa.wwords = a.wwords;
    sa.out_idx = out_idx + g0 * k;
    sa.out_score = out_score + g0 * k;
    const int e = L.large ? lk_run(la, s) : launch_select(sa, sel_tmp, s);
    if (e) return e;
  }
  if (out_member_p && n_members > 0) {
    size_t by = ((size_t)max_members * k + 255) / 256;
    if (by > 64) by = 64;
    with_width(dim, [&](auto kd) {
      hipLaunchKernelGGL(k_group_member_p<decltype(kd)::value>, dim3(n_groups, (unsigned)by), dim3(256), 0, s, a, out_idx, k,
                         out_member_p);
    });
    ANIREC_HIP_CHECK(hipGetLastError());
  }
  return ANIREC_OK;
}

// ------------------------------------------------------------------------------------
// the select alone, over score rows the caller holds (anirec_rows_topk): a third feeder.  Nothing is scored here, so
// a query's share of the workspace is the select's without a score row (none at all for k <= ANIREC_MAX_TOPK).
// ------------------------------------------------------------------------------------
size_t anirec_rows_topk_workspace_bytes(int32_t n, int32_t nq, int32_t k) {
  if (n < 1 || nq < 0 || k < 1) return 0;
  TopkLayout L = k <= ANIREC_MAX_TOPK ? select_layout(n) : lk_layout(n, k);
  L.per_query -= (size_t)n * 4;
  return L.bytes(nq < 1 ? 1 : nq, 4096);
}

int anirec_rows_topk(const float *scores, int64_t ld, int32_t n, int32_t nq, const int32_t *self, const uint8_t *keep,
                     const uint32_t *wbits, int32_t k, int32_t *out_idx, float *out_score, void *workspace,
                     size_t workspace_bytes, void *stream) {
  if (n < 1 || nq < 0 || k < 1 || ld < n) return ANIREC_EINVAL;
  if (nq == 0) return ANIREC_OK;
  if (!scores || !out_idx || !out_score || !workspace) return ANIREC_EINVAL;
  TopkLayout L = k <= ANIREC_MAX_TOPK ? select_layout(n) : lk_layout(n, k);
  L.per_query -= (size_t)n * 4;
  if (workspace_bytes < L.fixed + L.per_query) return ANIREC_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  size_t qb = L.per_query ? (workspace_bytes - L.fixed) / L.per_query : 4096;
  if (qb > 4096) qb = 4096;
  if (qb > (size_t)nq) qb = nq;
  LkArgs la = {};
  void *sel_tmp = nullptr;
  L.carve((char *)workspace, qb, la, sel_tmp);
  const int wwords = (n + 31) / 32;
  for (size_t q0 = 0; q0 < (size_t)nq; q0 += qb) {
    SelectArgs &sa = la.s;
    sa.scores = scores + q0 * (size_t)ld;
    sa.ld = (size_t)ld;
    sa.n = n;
    sa.nq = (int)((size_t)nq - q0 < qb ? (size_t)nq - q0 : qb);
    sa.k = k;
    sa.self = self ? self + q0 : nullptr;
    sa.keep = keep;
    sa.wbits = wbits ? wbits + q0 * wwords : nullptr;
    sa.wwords = wwords;
    sa.out_idx = out_idx + q0 * k;
    sa.out_score = out_score + q0 * k;
    const int e = L.large ? lk_run(la, s) : launch_select(sa, sel_tmp, s);
    if (e) return e;
  }
  return ANIREC_OK;
}

}  // extern "C"
