// Why an anime is in a list, for gfx950 (MI355X): include/anirec.h, anirec_explain_lists.  A list of k slots (rows of
// the normalised table What, -1 = empty) comes with a history (rows of What with a weight each, CSR); every present slot
// gets the m history entries with the largest contrib = weight * sim(slot, entry), ties to the lowest history position,
// NaN contribs never picked.  The order is total, so any split of the history gives the same picks.  The lists share
// nothing but the table: one workgroup per list,
//   check    every index of the list and of its history and the offsets pair are validated before anything is gathered
//            (a bad one: the list's outputs become -1 / NaN / NaN, *err = 1, nothing read through it).  The history
//            indices are 4 bytes an entry against 4 dim bytes a row: the pre-pass is cheap.
//   stage    the list's rows are gathered ONCE into LDS as float4 columns, img[v][c] = What[idx_c][4v .. 4v + 3], row pitch
//            P = k | 1 float4: k_listsim's image (8 lanes hold 8 consecutive v of one slot, conflict-free for odd P).
//   tiles    the history streams through a second image of T = anirec_explain_tile(dim, k) entries, himg[v][i], pitch
//            T | 1, filled the same way, the weights beside it.  The rows of the NEXT tile are loaded into registers
//            (8 float4 a lane) before the current tile's chains run, and stored to the image after its merge: the
//            gather's two dependent reads lie under the arithmetic.  Per tile:
//     chains   a lane takes one history entry against FOUR slots (4q .. 4q + 3): four k-ordered fma chains share five
//              ds_read_b128 per 16 fmas.  Lanes of consecutive entries read consecutive 16-byte slots of himg, lanes of one
//              q the same address of img (a broadcast).  Slot k of a short last quad is read as slot k - 1 and not
//              written.  Results go to sim[s][i] (pitch T | 1 floats).
//     merge    slot s belongs to `parts` = 256 / k lanes; lane p of them walks entries p, p + parts, ... of row s of sim
//              in ascending position and keeps its own sorted top-kM (kM = m rounded up to a power of two) in registers
//              across all tiles: a candidate enters where it is strictly larger, so equal contribs stay in position order.
//   join     the parts of a slot meet pairwise through LDS, log2(parts) rounds, under the full order (contrib
//            descending, position ascending); part 0 writes the slot's m ranks.
// LDS: image dim * (k | 1) floats (at most 16384 + dim: k <= anirec_explain_max_k(dim) = min(128, 16384 / dim)), history
// tile dim * (T | 1) with dim * T <= 8192, sim k * (T | 1) <= 8192 floats, the weights and the list's indices: 42 KiB
// for a list of 10 at width 128 (three workgroups a CU), 130 KiB at the longest list.  No workspace, no atomics; err is
// a plain store of the one value 1.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "anirec_dev.hpp"

namespace anirec {

constexpr int kExThreads = 256;
constexpr int kExImageFloats = 16384;  // dim * k at most ...
constexpr int kExMaxK = 128;           // ... and k at most this
constexpr int kExTileFloats = 8192;    // dim * T at most: the history tile
constexpr int kExSimFloats = 8192;     // k * (T | 1) at most: the tile's sim rows
constexpr int kExSlots = 4;            // slots a lane's history entry meets at once

typedef float ex_f4 __attribute__((ext_vector_type(4)));  // a float4 column piece held in registers

struct ExplainArgs {
  const float *What;        // [n_rows][dim] unit rows
  int n_rows;
  const int32_t *list_idx;  // [n_lists][k], -1 = empty slot
  int n_lists, k;
  const int64_t *off;       // [n_lists + 1]
  const int32_t *hidx;      // history rows
  const float *hw;          // history weights
  int m, tile;
  int scratch_floats;       // LDS floats of the history tile + sim rows / the join's lists (a multiple of 4)
  int32_t *out_pos;         // [n_lists][k][m]
  float *out_sim, *out_contrib;
  int32_t *err;
};

// host and device: the limits and the LDS layout
static inline __host__ __device__ int ex_max_k(int dim) {
  const int k = kExImageFloats / dim;
  return k < kExMaxK ? k : kExMaxK;
}
static inline __host__ __device__ int ex_tile(int dim, int k) {
  const int t = kExTileFloats / dim, u = (kExSimFloats / k - 1) & ~7;
  return t < u ? t : u;
}
static inline __host__ __device__ int ex_scratch_floats(int dim, int k, int tile) {
  const int f = (dim + k) * (tile | 1), j = kExThreads * ANIREC_EXPLAIN_MAX_M * 3;
  return ((f > j ? f : j) + 3) & ~3;
}
static inline __host__ __device__ size_t ex_lds_bytes(int dim, int k, int tile) {
  return ((size_t)dim * (k | 1) + ex_scratch_floats(dim, k, tile) + tile + k) * sizeof(float);
}

// One candidate into a sorted top-kM held in registers (empty ranks: pos -1 / NaN / NaN, at the end).  It enters at the
// first rank it beats and everything from there moves down one.  kFull: the whole order (contrib descending, position
// ascending); otherwise the candidate is known to stand after every entry held, and beats only a strictly smaller one.
template <int kM, bool kFull>
__device__ __forceinline__ void ex_insert(float (&tc)[kM], float (&ts)[kM], int (&tp)[kM], bool live, float c, float s,
                                          int p) {
  bool shift = false;
#pragma unroll
  for (int r = 0; r < kM; ++r) {
    bool better = live && (tp[r] < 0 || c > tc[r]);
    if constexpr (kFull) better = better || (live && c == tc[r] && p < tp[r]);
    shift = shift || better;
    const float oc = tc[r], os = ts[r];
    const int op = tp[r];
    tc[r] = shift ? c : oc;
    ts[r] = shift ? s : os;
    tp[r] = shift ? p : op;
    c = shift ? oc : c;
    s = shift ? os : s;
    p = shift ? op : p;
  }
}

// The pieces of one history tile into a lane's registers: piece j is float4 column (j % kVB) * 8 + (g & 7) of entry
// (g >> 3) + 32 (j / kVB).  A lane past the tile's last entry (tn >= 1 of them) loads that last entry again and stores
// nothing later: every piece is assigned, so the pieces stay in registers.
template <int kRowV, int kPre>
__device__ __forceinline__ void ex_fetch(ex_f4 (&pre)[kPre], float (&prew)[kPre / (kRowV / 8)], const float4 *W4,
                                         const int32_t *hidx, const float *hw, int tn, int g) {
  constexpr int kVB = kRowV / 8;
#pragma unroll
  for (int i = 0; i < kPre / kVB; ++i) {
    const int c = min((g >> 3) + (kExThreads / 8) * i, tn - 1);
    const int32_t h = hidx[c];
    prew[i] = hw[c];
#pragma unroll
    for (int u = 0; u < kVB; ++u)
      pre[i * kVB + u] = reinterpret_cast<const ex_f4 *>(W4)[(size_t)h * kRowV + u * 8 + (g & 7)];
  }
}

template <int kD, int kM>
__global__ __launch_bounds__(kExThreads) void k_explain(ExplainArgs a) {
  constexpr int kRowV = kD / 4;  // float4 per row
  extern __shared__ __attribute__((aligned(16))) float ex_smem[];
  const int g = threadIdx.x, k = a.k, m = a.m, T = a.tile;
  const int P = k | 1, PT = T | 1;
  const long long l = blockIdx.x;
  float4 *img = reinterpret_cast<float4 *>(ex_smem);      // [kRowV][P]
  float *scratch = ex_smem + (size_t)kD * P;
  float4 *himg = reinterpret_cast<float4 *>(scratch);     // [kRowV][PT]
  float *sim = scratch + (size_t)kD * PT;                 // [k][PT]
  float *wt = scratch + a.scratch_floats;                 // [T]
  int32_t *row_of = reinterpret_cast<int32_t *>(wt + T);  // [k] table row, -1 = empty
  const int32_t *lidx = a.list_idx + l * k;
  const long long obase = l * k * m;
  const float nanv = __uint_as_float(0x7FC00000u);
  const float4 *W4 = reinterpret_cast<const float4 *>(a.What);

  // check: nothing is read through an index or an offset before the whole list and its history have passed
  int bad = 0;
  for (int c = g; c < k; c += kExThreads) {
    const int32_t r = lidx[c];
    bad |= (r < -1 || r >= a.n_rows);
    row_of[c] = r;
  }
  const long long o0 = a.off[l], o1 = a.off[l + 1];
  const bool offbad = o0 < 0 || o1 < o0 || o1 - o0 > (long long)INT_MAX;
  bad |= offbad;
  const int n = offbad ? 0 : (int)(o1 - o0);
  for (long long i = g; i < n; i += kExThreads) {
    const int32_t h = a.hidx[o0 + i];
    bad |= (h < 0 || h >= a.n_rows);
  }
  bad = __syncthreads_or(bad);
  if (bad) {
    if (g == 0) *a.err = 1;
    for (int e = g; e < k * m; e += kExThreads) {
      a.out_pos[obase + e] = -1;
      a.out_sim[obase + e] = nanv;
      a.out_contrib[obase + e] = nanv;
    }
    return;
  }

  // A tile's rows travel through registers: piece j of a lane is float4 column (j % kVB) * 8 + (g & 7) of entry
  // (g >> 3) + 32 (j / kVB) — the stage's pattern, kPre pieces cover dim * T <= 8192 floats — and the pieces of the
  // NEXT tile are loaded (index, then row: two dependent reads) before the chains of the current one run, so that
  // their latency lies under the chains and the merge instead of in front of a barrier (the first tile's: under the
  // stage of the list's own rows).
  constexpr int kVB = kRowV / 8, kPre = kExTileFloats / 4 / kExThreads;
  static_assert(kPre % kVB == 0, "a tile is a whole number of 32-entry passes");
  ex_f4 pre[kPre];
  float prew[kPre / kVB];
  if (n > 0) ex_fetch<kRowV, kPre>(pre, prew, W4, a.hidx + o0, a.hw + o0, (int)((long long)T < n ? (long long)T : n), g);

  // stage: 8 lanes hold 8 consecutive float4 columns of one slot, 32 slots a pass
  for (int vb = 0; vb < kRowV; vb += 8) {
    const int v = vb + (g & 7);
    for (int c = g >> 3; c < k; c += kExThreads / 8) {
      const int32_t r = row_of[c];
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r >= 0) x = W4[(size_t)r * kRowV + v];
      img[v * P + c] = x;
    }
  }

  // this lane's share of the merge: part p_own of slot s_own
  const int parts = kExThreads / k;  // >= 2: k <= 128
  const int s_own = g / parts, p_own = g - s_own * parts;
  const bool own = s_own < k;
  const bool present = own && row_of[s_own] >= 0;
  float tc[kM], ts[kM];
  int tp[kM];
#pragma unroll
  for (int r = 0; r < kM; ++r) {
    tc[r] = nanv;
    ts[r] = nanv;
    tp[r] = -1;
  }

  const int nq = (k + kExSlots - 1) / kExSlots;
  for (long long base = 0; base < n; base += T) {
    const int tcur = (int)((long long)T < n - base ? (long long)T : n - base);
    // the tile's pieces into the history image (the last merge is behind a barrier)
#pragma unroll
    for (int j = 0; j < kPre; ++j) {
      const int v = (j % kVB) * 8 + (g & 7), c = (g >> 3) + (kExThreads / 8) * (j / kVB);
      if (c < tcur) {
        reinterpret_cast<ex_f4 *>(himg)[v * PT + c] = pre[j];
        if (j % kVB == 0 && (g & 7) == 0) wt[c] = prew[j / kVB];
      }
    }
    __syncthreads();
    if (base + T < n) {
      const long long rest = n - (base + T);
      ex_fetch<kRowV, kPre>(pre, prew, W4, a.hidx + o0 + base + T, a.hw + o0 + base + T,
                            (int)((long long)T < rest ? (long long)T : rest), g);
    }
    // chains: history entry i against slots 4q .. 4q + 3
    for (int e = g; e < nq * tcur; e += kExThreads) {
      const int q = e / tcur, i = e - q * tcur;
      const int s0 = kExSlots * q, s1 = min(s0 + 1, k - 1), s2 = min(s0 + 2, k - 1), s3 = min(s0 + 3, k - 1);
      const float4 *p0 = img + s0, *p1 = img + s1, *p2 = img + s2, *p3 = img + s3, *ph = himg + i;
      float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
#pragma unroll 4
      for (int v = 0; v < kRowV; ++v) {
        const float4 y = ph[v * PT], x0 = p0[v * P], x1 = p1[v * P], x2 = p2[v * P], x3 = p3[v * P];
        c0 = __fmaf_rn(x0.x, y.x, c0);
        c1 = __fmaf_rn(x1.x, y.x, c1);
        c2 = __fmaf_rn(x2.x, y.x, c2);
        c3 = __fmaf_rn(x3.x, y.x, c3);
        c0 = __fmaf_rn(x0.y, y.y, c0);
        c1 = __fmaf_rn(x1.y, y.y, c1);
        c2 = __fmaf_rn(x2.y, y.y, c2);
        c3 = __fmaf_rn(x3.y, y.y, c3);
        c0 = __fmaf_rn(x0.z, y.z, c0);
        c1 = __fmaf_rn(x1.z, y.z, c1);
        c2 = __fmaf_rn(x2.z, y.z, c2);
        c3 = __fmaf_rn(x3.z, y.z, c3);
        c0 = __fmaf_rn(x0.w, y.w, c0);
        c1 = __fmaf_rn(x1.w, y.w, c1);
        c2 = __fmaf_rn(x2.w, y.w, c2);
        c3 = __fmaf_rn(x3.w, y.w, c3);
      }
      float *d = sim + s0 * PT + i;
      d[0] = c0;
      if (s0 + 1 < k) d[PT] = c1;
      if (s0 + 2 < k) d[2 * PT] = c2;
      if (s0 + 3 < k) d[3 * PT] = c3;
    }
    __syncthreads();
    // merge: ascending position within the lane, so a tie never displaces
    if (present) {
      const float *srow = sim + s_own * PT;
      for (int i = p_own; i < tcur; i += parts) {
        const float sv = srow[i];
        const float c = __fmul_rn(wt[i], sv);
        ex_insert<kM, false>(tc, ts, tp, c == c, c, sv, (int)(base + i));
      }
    }
    __syncthreads();
  }

  // join: part p takes in part p + stride, stride = 1, 2, 4, ...; lane g's list lies at fin[g] (the tile is done with)
  float *fin_c = scratch, *fin_s = scratch + kExThreads * kM;
  int *fin_p = reinterpret_cast<int *>(scratch + 2 * kExThreads * kM);
  for (int stride = 1; stride < parts; stride <<= 1) {
    const int mask = 2 * stride - 1;
    if (own && (p_own & mask) == stride) {
#pragma unroll
      for (int r = 0; r < kM; ++r) {
        fin_c[g * kM + r] = tc[r];
        fin_s[g * kM + r] = ts[r];
        fin_p[g * kM + r] = tp[r];
      }
    }
    __syncthreads();
    if (own && (p_own & mask) == 0 && p_own + stride < parts) {
      const int o = (g + stride) * kM;
#pragma unroll
      for (int r = 0; r < kM; ++r) {
        const int pp = fin_p[o + r];
        ex_insert<kM, true>(tc, ts, tp, pp >= 0, fin_c[o + r], fin_s[o + r], pp);
      }
    }
    __syncthreads();
  }

  if (own && p_own == 0) {
    const long long ob = obase + (long long)s_own * m;
#pragma unroll
    for (int r = 0; r < kM; ++r) {
      if (r < m) {
        a.out_pos[ob + r] = tp[r];
        a.out_sim[ob + r] = ts[r];
        a.out_contrib[ob + r] = tc[r];
      }
    }
  }
}

}  // namespace anirec

using namespace anirec;

extern "C" {

size_t anirec_explain_max_k(int32_t dim) { return dim_ok(dim) ? (size_t)ex_max_k(dim) : 0; }

size_t anirec_explain_tile(int32_t dim, int32_t k) {
  if (!dim_ok(dim) || k < 1 || k > ex_max_k(dim)) return 0;
  return (size_t)ex_tile(dim, k);
}

int anirec_explain_lists(const float *What, int32_t dim, int32_t n_rows, const int32_t *list_idx, int32_t n_lists,
                         int32_t k, const int64_t *hist_offsets, const int32_t *hist_idx, const float *hist_weight,
                         int32_t m, int32_t *out_pos, float *out_sim, float *out_contrib, int32_t *err_flag,
                         void *stream) {
  if (!dim_ok(dim) || n_rows < 1 || n_lists < 0 || k < 1 || k > ex_max_k(dim) || m < 1 || m > ANIREC_EXPLAIN_MAX_M)
    return ANIREC_EINVAL;
  if (n_lists == 0) return ANIREC_OK;
  if (!What || !list_idx || !hist_offsets || !out_pos || !out_sim || !out_contrib || !err_flag) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ExplainArgs a;
  a.What = What;
  a.n_rows = n_rows;
  a.list_idx = list_idx;
  a.n_lists = n_lists;
  a.k = k;
  a.off = hist_offsets;
  a.hidx = hist_idx;
  a.hw = hist_weight;
  a.m = m;
  a.tile = ex_tile(dim, k);
  a.scratch_floats = ex_scratch_floats(dim, k, a.tile);
  a.out_pos = out_pos;
  a.out_sim = out_sim;
  a.out_contrib = out_contrib;
  a.err = err_flag;
  const size_t lds = ex_lds_bytes(dim, k, a.tile);
  int status = ANIREC_OK;
  with_width(dim, [&](auto kd) {
    constexpr int kD = decltype(kd)::value;
    const auto launch = [&](auto kernel) {
      hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e == hipSuccess) e = hipMemsetAsync(err_flag, 0, sizeof(int32_t), s);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_lists), dim3(kExThreads), lds, s, a);
        e = hipGetLastError();
      }
      status = (int)e;
    };
    if (m <= 1) {
      launch(k_explain<kD, 1>);
    } else if (m <= 2) {
      launch(k_explain<kD, 2>);
    } else if (m <= 4) {
      launch(k_explain<kD, 4>);
    } else {
      launch(k_explain<kD, 8>);
    }
  });
  return status;
}

}  // extern "C"
