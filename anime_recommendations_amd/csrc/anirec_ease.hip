// EASE (Steck 2019) for gfx950 (MI355X): include/anirec.h, anirec_spd_inverse / anirec_ease_weights /
// anirec_ease_scores.  DESIGN.md 4.24.
//
// THE INVERSE is a blocked Gauss-Jordan elimination in place, without pivoting (A is symmetric positive definite, so
// every diagonal block met on the way is), NB = kNB = 64, T = ceil(n / NB) block steps.  Block step b, with
// K = [b NB, min(n, (b + 1) NB)) and every block padded to NB x NB (the diagonal block with the identity, every other
// block with zeros; no padded element is read from or written to A):
//   1  k_ease_diag   ONE workgroup loads D = A[K][K] into LDS and inverts it by the unblocked form of the same
//                    elimination: for p = 0 .. NB-1 in order, with t = 1 / D[p][p] (one correctly rounded divide),
//                      row[j] = D[p][j] * t (j != p),  col[i] = D[i][p] (i != p)
//                      D[i][j] = fma(-col[i], row[j], D[i][j])   (i != p, j != p)
//                      D[p][j] = row[j],   D[i][p] = -(col[i] * t),   D[p][p] = t
//                    A pivot D[p][p] that is not > 0 or not finite makes *info = b + 1 unless it is set already; the
//                    arithmetic goes on with what it has (the loops do not depend on the values).  R = the result.
//   2  k_ease_panel  one workgroup per block column t:  Rp[:, t] = (t == b) ? R : R . A[K][t]  (NB x NB by NB x NB, the
//                    sum over k = 0 .. NB-1 in order, one fma a term, from 0), and the column panel negated and
//                    transposed, Cn[:, t] = (t == b) ? +I : -(A[t][K])^T.  Both are [NB][T NB] on the workspace.
//   3  k_ease_update one workgroup per NB x NB tile (I, J) of A:  A[I][J] = Base + Cn[:, I]^T . Rp[:, J], where Base is
//                    A[I][J], or 0 when I == b or J == b.  So the block row becomes R . A[K][J], the block column
//                    -A[I][K] . R, the diagonal block R, and every other tile A[I][J] - A[I][K] . R . A[K][J].  The sum
//                    over k runs through v_mfma_f64_16x16x4_f64, four k to an instruction, k ascending, accumulated
//                    onto Base; a lane owns its output elements, nothing is added across lanes or workgroups.
// After the T steps A holds its inverse.  The bits are a function of A, n and ld: every workspace element that is read
// was written by the same call, and every output element has one owner and one order.
//
// f64 MFMA operands (the C/D map differs from every other dtype's): lane l gives A[row l & 15][k l >> 4] and
// B[k l >> 4][col l & 15]; it holds D[row (l >> 4) + 4 r][col l & 15] in register pair r = 0 .. 3.
// Both panels are staged k-major in LDS, half of NB at a time (32 KiB), element (k, c) at k * 64 + (c ^ ((k & 1) << 4)):
// the two k of a 32-lane half of a ds_read_b64 fall on the two halves of the 64 banks.
//
// THE WEIGHTS are one correctly rounded divide and one rounding to fp32 an element; THE SCORE ROWS are int64 sums of
// fixed-point terms (the term rule of anirec_itemknn_scores), one thread per output element: column tile the slow grid
// index, so that the workgroups in flight read one slab of W; a list's entries staged in LDS kEaseEntries at a time.
#include <hip/hip_runtime.h>
#include <math.h>

#include "anirec_dev.hpp"

namespace anirec {

constexpr int kNB = 64;                 // anirec_spd_inverse_block(): block size, tile size of every kernel below
constexpr int kEaseColTile = 1024;      // columns of one workgroup of k_ease_scores (256 threads x 4)
constexpr int kEaseEntries = 512;       // history entries staged in LDS at a time
constexpr double kEaseScale = 1073741824.0;  // 2^30
constexpr double kEaseInvScale = 1.0 / 1073741824.0;
constexpr double kEaseMaxTerm = 1024.0;
constexpr double kEaseMagic = 6755399441055744.0;  // 1.5 * 2^52: x + magic holds rint(x) in its low bits, |x| < 2^51

typedef double double4_t __attribute__((ext_vector_type(4)));

static inline size_t ease_npad(int32_t n) { return ((size_t)n + kNB - 1) / kNB * kNB; }

__global__ __launch_bounds__(256) void k_ease_diag(const double *__restrict__ A, int64_t ld, int n, int b,
                                                   double *__restrict__ R, int32_t *__restrict__ info) {
  __shared__ double D[kNB][kNB + 1];
  __shared__ double row[kNB], col[kNB];
  __shared__ int fail;
  const int tid = threadIdx.x;
  const int64_t k0 = (int64_t)b * kNB;
  if (tid == 0) fail = 0;
  for (int e = tid; e < kNB * kNB; e += 256) {
    const int i = e >> 6, j = e & 63;
    const int64_t gi = k0 + i, gj = k0 + j;
    D[i][j] = (gi < n && gj < n) ? A[gi * ld + gj] : (i == j ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int p = 0; p < kNB; ++p) {
    const double piv = D[p][p];
    const double t = 1.0 / piv;
    if (tid < kNB) {
      row[tid] = D[p][tid] * t;
      col[tid] = D[tid][p];
      if (tid == 0 && !(piv > 0.0 && piv <= 1.79769313486231570815e+308)) fail = 1;
    }
    __syncthreads();
    for (int e = tid; e < kNB * kNB; e += 256) {
      const int i = e >> 6, j = e & 63;
      double v;
      if (i == p) {
        v = j == p ? t : row[j];
      } else if (j == p) {
        v = -(col[i] * t);
      } else {
        v = fma(-col[i], row[j], D[i][j]);
      }
      D[i][j] = v;
    }
    __syncthreads();
  }
  for (int e = tid; e < kNB * kNB; e += 256) R[e] = D[e >> 6][e & 63];
  if (tid == 0 && fail && *info == 0) *info = b + 1;
}

__global__ __launch_bounds__(256) void k_ease_panel(const double *__restrict__ A, int64_t ld, int n, int b,
                                                    const double *__restrict__ R, double *__restrict__ Rp,
                                                    double *__restrict__ Cn, int64_t npad) {
  __shared__ double sR[kNB][kNB];      // R[i][k]: read as a broadcast
  __shared__ double sX[kNB][kNB + 1];  // A[K][t] as [k][j], then A[t][K] as [i][k]
  const int tid = threadIdx.x;
  const int t = blockIdx.x;
  const int64_t k0 = (int64_t)b * kNB, t0 = (int64_t)t * kNB;
  if (t == b) {
    for (int e = tid; e < kNB * kNB; e += 256) {
      const int k = e >> 6, c = e & 63;
      Rp[(int64_t)k * npad + t0 + c] = R[e];
      Cn[(int64_t)k * npad + t0 + c] = k == c ? 1.0 : 0.0;
    }
    return;
  }
  for (int e = tid; e < kNB * kNB; e += 256) {
    const int k = e >> 6, c = e & 63;
    const int64_t gk = k0 + k, gc = t0 + c;
    sR[k][c] = R[e];
    sX[k][c] = (gk < n && gc < n) ? A[gk * ld + gc] : 0.0;
  }
  __syncthreads();
  {
    const int j = tid & 63, i0 = (tid >> 6) * 16;
    double acc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0;
    for (int k = 0; k < kNB; ++k) {
      const double x = sX[k][j];
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = fma(sR[i0 + r][k], x, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) Rp[(int64_t)(i0 + r) * npad + t0 + j] = acc[r];
  }
  __syncthreads();
  for (int e = tid; e < kNB * kNB; e += 256) {  // rows i of block t, columns K: read along k
    const int i = e >> 6, k = e & 63;
    const int64_t gi = t0 + i, gk = k0 + k;
    sX[i][k] = (gi < n && gk < n) ? -A[gi * ld + gk] : 0.0;
  }
  __syncthreads();
  for (int e = tid; e < kNB * kNB; e += 256) {
    const int k = e >> 6, i = e & 63;
    Cn[(int64_t)k * npad + t0 + i] = sX[i][k];
  }
}

__device__ __forceinline__ int ease_lds_at(int k, int c) { return k * kNB + (c ^ ((k & 1) << 4)); }

__global__ __launch_bounds__(256) void k_ease_update(double *__restrict__ A, int64_t ld, int n, int b,
                                                     const double *__restrict__ Rp, const double *__restrict__ Cn,
                                                     int64_t npad) {
  __shared__ double sA[(kNB / 2) * kNB];
  __shared__ double sB[(kNB / 2) * kNB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tj = blockIdx.x, ti = blockIdx.y;
  const int64_t i0 = (int64_t)ti * kNB, j0 = (int64_t)tj * kNB;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
  const int lr = lane >> 4, lc = lane & 15;
  const bool fresh = ti == b || tj == b;  // the block row and the block column start from 0
  double4_t acc[2][2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t gi = i0 + wr + rt * 16 + lr + 4 * r, gj = j0 + wc + ct * 16 + lc;
        acc[rt][ct][r] = (!fresh && gi < n && gj < n) ? A[gi * ld + gj] : 0.0;
      }
  for (int h = 0; h < 2; ++h) {
    if (h) __syncthreads();
    for (int e = tid; e < (kNB / 2) * kNB; e += 256) {
      const int k = e >> 6, c = e & 63;
      const int64_t g = (int64_t)(h * (kNB / 2) + k) * npad;
      sA[ease_lds_at(k, c)] = Cn[g + i0 + c];
      sB[ease_lds_at(k, c)] = Rp[g + j0 + c];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kNB / 2; kk += 4) {
      double a[2], bv[2];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) a[rt] = sA[ease_lds_at(kk + lr, wr + rt * 16 + lc)];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) bv[ct] = sB[ease_lds_at(kk + lr, wc + ct * 16 + lc)];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
          acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rt], bv[ct], acc[rt][ct], 0, 0, 0);
    }
  }
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t gi = i0 + wr + rt * 16 + lr + 4 * r, gj = j0 + wc + ct * 16 + lc;
        if (gi < n && gj < n) A[gi * ld + gj] = acc[rt][ct][r];
      }
}

__global__ __launch_bounds__(256) void k_ease_weights(const double *__restrict__ P, int64_t ldp, int n,
                                                      float *__restrict__ W, int64_t ldw) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double d = P[j * ldp + j];
  for (int64_t i = blockIdx.y; i < n; i += gridDim.y)
    W[i * ldw + j] = i == j ? 0.0f : (float)__ddiv_rn(-P[i * ldp + j], d);
}

struct EaseArgs {
  const float *W;
  int64_t ldw;
  int n_items;
  const int32_t *offsets;
  const int32_t *hist_idx;
  const float *hist_w;  // optional
  int n_hist;
  float *out;
  int64_t ld;
  int32_t *err;
};

__global__ __launch_bounds__(256) void k_ease_scores(EaseArgs a) {
  __shared__ int32_t s_idx[kEaseEntries];
  __shared__ float s_w[kEaseEntries];
  const int tid = threadIdx.x;
  const int64_t l = blockIdx.x;
  float *out = a.out + l * a.ld;
  const int lo = a.offsets[l], hi = a.offsets[l + 1];
  const int n_tiles = (a.n_items + kEaseColTile - 1) / kEaseColTile;
  if (lo < 0 || hi < lo || hi > a.n_hist) {  // a bad pair: the row is NaN, nothing is read through it
    if (tid == 0 && blockIdx.y == 0) *a.err = 1;
    for (int t = blockIdx.y; t < n_tiles; t += gridDim.y)
      for (int c = 0; c < 4; ++c) {
        const int64_t j = (int64_t)t * kEaseColTile + c * 256 + tid;
        if (j < a.n_items) out[j] = __uint_as_float(0x7FC00000u);
      }
    return;
  }
  bool bad = false;
  for (int t = blockIdx.y; t < n_tiles; t += gridDim.y) {
    const int64_t jb = (int64_t)t * kEaseColTile + tid;
    long long S[4] = {0, 0, 0, 0};
    for (int e0 = lo; e0 < hi; e0 += kEaseEntries) {
      const int ne = hi - e0 < kEaseEntries ? hi - e0 : kEaseEntries;
      __syncthreads();  // the tile before this one has been read
      for (int e = tid; e < ne; e += 256) {
        int i = a.hist_idx[e0 + e];
        if ((uint32_t)i >= (uint32_t)a.n_items) {  // the entry adds nothing; nothing is read through it
          i = -1;
          bad = true;
        }
        s_idx[e] = i;
        s_w[e] = a.hist_w ? a.hist_w[e0 + e] : 1.0f;
      }
      __syncthreads();
      for (int e = 0; e < ne; ++e) {
        const int i = s_idx[e];
        if (i < 0) continue;
        const double w = (double)s_w[e];
        const float *wrow = a.W + (int64_t)i * a.ldw;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int64_t j = jb + c * 256;
          if (j >= a.n_items) continue;
          const double prod = w * (double)wrow[j];  // exact: two 24-bit significands
          if (!(fabs(prod) <= kEaseMaxTerm)) {      // NaN, an infinite factor or a term past the documented range
            bad = true;
            continue;
          }
          // llrint(prod * 2^30): the scaling is exact and |.| <= 2^40, so the sum with 1.5 * 2^52 rounds it to the
          // nearest even integer and holds that in its low bits
          const double m = prod * kEaseScale + kEaseMagic;
          S[c] += __double_as_longlong(m) - __double_as_longlong(kEaseMagic);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t j = jb + c * 256;
      if (j < a.n_items) out[j] = (float)((double)S[c] * kEaseInvScale);
    }
  }
  if (bad) *a.err = 1;
}

}  // namespace anirec

using namespace anirec;

extern "C" {

int32_t anirec_spd_inverse_block(void) { return kNB; }
int32_t anirec_ease_scores_col_tile(void) { return kEaseColTile; }
int32_t anirec_ease_scores_entry_tile(void) { return kEaseEntries; }

size_t anirec_spd_inverse_workspace_bytes(int32_t n) {
  if (n < 1) return 0;
  return (size_t)kNB * kNB * 8 + 2 * (size_t)kNB * ease_npad(n) * 8;
}

int anirec_spd_inverse(double *A_inout, int64_t ld, int32_t n, int32_t *info, void *ws, size_t ws_bytes,
                       void *stream) {
  if (n < 1 || ld < (int64_t)n || !A_inout || !info || !ws) return ANIREC_EINVAL;
  if (((uintptr_t)A_inout & 7u) || ((uintptr_t)ws & 7u) || ((uintptr_t)info & 3u)) return ANIREC_EINVAL;
  if (ws_bytes < anirec_spd_inverse_workspace_bytes(n)) return ANIREC_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int64_t npad = (int64_t)ease_npad(n);
  const int T = (int)(npad / kNB);
  if (T > 65535) return ANIREC_EINVAL;  // grid.y of the update; n <= 4 194 240
  double *R = (double *)ws, *Rp = R + kNB * kNB, *Cn = Rp + (size_t)kNB * npad;
  ANIREC_HIP_CHECK(hipMemsetAsync(info, 0, 4, s));
  for (int b = 0; b < T; ++b) {
    hipLaunchKernelGGL(k_ease_diag, dim3(1), dim3(256), 0, s, A_inout, ld, n, b, R, info);
    hipLaunchKernelGGL(k_ease_panel, dim3(T), dim3(256), 0, s, A_inout, ld, n, b, R, Rp, Cn, npad);
    hipLaunchKernelGGL(k_ease_update, dim3(T, T), dim3(256), 0, s, A_inout, ld, n, b, Rp, Cn, npad);
  }
  return (int)hipGetLastError();
}

int anirec_ease_weights(const double *P, int64_t ldp, int32_t n, float *W_out, int64_t ldw, void *stream) {
  if (n < 1 || ldp < (int64_t)n || ldw < (int64_t)n || !P || !W_out) return ANIREC_EINVAL;
  if (((uintptr_t)P & 7u) || ((uintptr_t)W_out & 3u)) return ANIREC_EINVAL;
  const unsigned gx = ((unsigned)n + 255u) / 256u;
  const unsigned gy = n < 1024 ? (unsigned)n : 1024u;
  hipLaunchKernelGGL(k_ease_weights, dim3(gx, gy), dim3(256), 0, (hipStream_t)stream, P, ldp, n, W_out, ldw);
  return (int)hipGetLastError();
}

int anirec_ease_scores(const float *W, int64_t ldw, int32_t n_items, const int32_t *hist_offsets,
                       const int32_t *hist_idx, const float *hist_w, int32_t n_lists, int32_t n_hist,
                       float *out_scores, int64_t ld, int32_t *err_flag, void *stream) {
  if (n_items < 1 || n_lists < 0 || n_hist < 0 || ldw < (int64_t)n_items || ld < (int64_t)n_items)
    return ANIREC_EINVAL;
  if (n_lists == 0) return ANIREC_OK;
  if (!W || !hist_offsets || !out_scores || !err_flag || (n_hist > 0 && !hist_idx)) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  EaseArgs a;
  a.W = W;
  a.ldw = ldw;
  a.n_items = n_items;
  a.offsets = hist_offsets;
  a.hist_idx = hist_idx;
  a.hist_w = hist_w;
  a.n_hist = n_hist;
  a.out = out_scores;
  a.ld = ld;
  a.err = err_flag;
  const unsigned tiles = ((unsigned)n_items + kEaseColTile - 1) / kEaseColTile;
  hipLaunchKernelGGL(k_ease_scores, dim3((unsigned)n_lists, tiles < 65535u ? tiles : 65535u), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

}  // extern "C"
