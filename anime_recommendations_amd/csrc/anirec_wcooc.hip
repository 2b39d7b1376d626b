// User-weighted co-occurrence on the i8 matrix cores, for gfx950 (MI355X): include/anirec.h, anirec_wcooc_scores.
// S[q][j] = the sum of an integer weight q_u (0 .. ANIREC_WCOOC_MAX_Q, 14 bits) over the users set in both bit rows.
// Everything up to S is a sum of INTEGERS: q_u is split into two 7-bit limbs (lo = q & 127, hi = q >> 7, both valid
// signed bytes), one operand of v_mfma_i32_16x16x64_i8 holds the query's 0/1 bits ANDed with a limb, the other the
// key's plain 0/1 bits, and each limb has its own int32 accumulators: 127 * 2^24 < 2^31, so with n_users <= 2^24 no
// accumulator can wrap and S = hi * 128 + lo is exact in int64, whatever the order the products are added in.
//   split      k_wcooc_split: validates user_q (outside 0 .. MAX_Q counts as 0 and raises the flag) and writes the two
//              limb byte arrays to the workspace, four users a thread, padded with zeros to a whole chunk of users.
//   sums       k_wcooc: a 256-thread workgroup owns 64 queries x 64 keys, a wave 32 x 32 of them as 2 x 2 MFMA tiles.
//              Per pass it stages kWChunk = 64 user words of both row sets in LDS as k_cooc does (pitch 68 words: the
//              16 rows x 2 word pairs of a 32-lane ds_read_b64 group start at banks 4 r + 2 g, all distinct), the
//              last word of a row masked, rows past the edge and rows of a bad query zero, and beside them the 2048
//              lo and hi bytes of the chunk's users.  A step covers 256 users: lane (r = l & 15, g = l >> 4) reads the
//              word pair 2 g, 2 g + 1 of its rows (64 users) and the 64 + 64 limb bytes of those users, and feeds four
//              MFMAs, the m-th with the m-th 16 users of its 64.  The hardware's k order inside an instruction does
//              not matter: the sum over k is the same under any permutation applied to both operands alike, and both
//              fragments (and the limb bytes) are built from the same users in the same byte positions.  Four bits
//              become four 0/1 bytes t by (nibble * 0x00204081) & 0x01010101; (0x80808080 - t) has 0x7F in the bytes
//              of set bits and 0x80 in the others, so ANDed with four packed 7-bit limb bytes it is the weighted
//              operand (no full-width multiply).  An expanded fragment feeds two tiles (and the mask both limbs).
//   epilogue   S -> weight: two fp64 multiplies rounded one by one (nothing contracted), one rounding to fp32; the
//              excl words of a tile are put together in LDS and stored whole, as in k_cooc.
#include <hip/hip_runtime.h>
#include <math.h>

#include "anirec_dev.hpp"

namespace anirec {

constexpr int kWTile = 64;     // queries and keys of one workgroup
constexpr int kWChunk = 64;    // user words staged per pass (anirec_wcooc_chunk_words)
constexpr int kWPitch = 68;    // words between staged rows
constexpr int kWChunkUsers = kWChunk * 32;
constexpr int kWMaxUsers = 1 << 24;

typedef int v4i __attribute__((ext_vector_type(4)));

struct WCoocArgs {
  const uint32_t *bits;   // [n_items][W]
  int n_items, W;
  uint32_t last_mask;     // the valid bits of word W - 1
  const int32_t *queries; // [nq]
  int nq;
  const uint32_t *lo, *hi;  // limb bytes (workspace), four users a word, whole chunks
  const double *row_scale, *col_scale;
  float *out_w;           // [nq][n_items]
  long long *out_sum;     // optional [nq][n_items]
  uint32_t *out_excl;     // optional [nq][ewords]
  int ewords;
  int32_t *err;
};

__global__ __launch_bounds__(256) void k_wcooc_split(const int32_t *__restrict__ user_q, int n_users, int n_pad,
                                                     uint32_t *__restrict__ lo, uint32_t *__restrict__ hi,
                                                     int32_t *__restrict__ err) {
  const int g = blockIdx.x * 256 + threadIdx.x;  // four users
  if (g * 4 >= n_pad) return;
  uint32_t l = 0u, h = 0u;
  bool bad = false;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int u = g * 4 + b;
    int q = u < n_users ? user_q[u] : 0;
    if ((uint32_t)q > (uint32_t)ANIREC_WCOOC_MAX_Q) {
      q = 0;
      bad = true;
    }
    l |= (uint32_t)(q & 127) << (8 * b);
    h |= (uint32_t)(q >> 7) << (8 * b);
  }
  lo[g] = l;
  hi[g] = h;
  if (bad) *err = 1;
}

// four bits -> four 0/1 bytes (bit b of the nibble in byte b)
__device__ __forceinline__ uint32_t nib01(uint32_t bits16, int n) {
  return (((bits16 >> (4 * n)) & 15u) * 0x00204081u) & 0x01010101u;
}

__device__ __forceinline__ float wcooc_weight(long long s, double rs, double cs) {
#pragma clang fp contract(off)
  const double a = (double)s * rs;
  return (float)(a * cs);
}

__global__ __launch_bounds__(256) void k_wcooc(WCoocArgs a) {
  __shared__ __align__(16) uint32_t sq[kWTile * kWPitch];
  __shared__ __align__(16) uint32_t sk[kWTile * kWPitch];
  __shared__ __align__(16) uint32_t slo[kWChunkUsers / 4];
  __shared__ __align__(16) uint32_t shi[kWChunkUsers / 4];
  __shared__ int qrow[kWTile];
  __shared__ uint32_t ex[kWTile][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int wq = (wave >> 1) * 32, wk = (wave & 1) * 32;  // the wave's 32 x 32 corner of the tile
  const int j0 = blockIdx.x * kWTile, q0 = blockIdx.y * kWTile;
  if (tid < kWTile) {
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
  v4i alo[2][2], ahi[2][2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      alo[rt][ct] = v4i{0, 0, 0, 0};
      ahi[rt][ct] = v4i{0, 0, 0, 0};
    }

  for (int w0 = 0; w0 < a.W; w0 += kWChunk) {
#pragma unroll 4
    for (int i = tid; i < kWTile * kWChunk; i += 256) {
      const int rr = i >> 6, w = i & 63, gw = w0 + w;
      uint32_t vq = 0u, vk = 0u;
      if (gw < a.W) {
        const uint32_t m = gw == a.W - 1 ? a.last_mask : 0xFFFFFFFFu;
        const int qr = qrow[rr], j = j0 + rr;
        if (qr >= 0) vq = a.bits[(size_t)qr * a.W + gw] & m;
        if (j < a.n_items) vk = a.bits[(size_t)j * a.W + gw] & m;
      }
      sq[rr * kWPitch + w] = vq;
      sk[rr * kWPitch + w] = vk;
    }
    {  // the limb arrays hold whole chunks: no edge
      const size_t base = (size_t)w0 * 8;  // words of four users
      slo[tid] = a.lo[base + tid];
      slo[tid + 256] = a.lo[base + tid + 256];
      shi[tid] = a.hi[base + tid];
      shi[tid + 256] = a.hi[base + tid + 256];
    }
    __syncthreads();
    const int wl = a.W - w0 < kWChunk ? a.W - w0 : kWChunk;  // words past wl are staged zeros
    for (int w = 0; w < wl; w += 8) {
      uint2 qv[2], kv[2];
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) qv[rt] = *(const uint2 *)&sq[(wq + 16 * rt + r) * kWPitch + w + 2 * g];
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) kv[ct] = *(const uint2 *)&sk[(wk + 16 * ct + r) * kWPitch + w + 2 * g];
      const int lw = (w + 2 * g) * 8;  // the first limb word of the lane's 64 users
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const uint4 l4 = *(const uint4 *)&slo[lw + 4 * m];
        const uint4 h4 = *(const uint4 *)&shi[lw + 4 * m];
        const uint32_t lw4[4] = {l4.x, l4.y, l4.z, l4.w}, hw4[4] = {h4.x, h4.y, h4.z, h4.w};
        v4i fl[2], fh[2], fb[2];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
          const uint32_t b16 = ((m < 2 ? qv[rt].x : qv[rt].y) >> (16 * (m & 1))) & 0xFFFFu;
#pragma unroll
          for (int n = 0; n < 4; ++n) {
            // 0x80 - 0 = 0x80 keeps nothing of a 7-bit limb, 0x80 - 1 = 0x7F all of it; no byte borrows
            const uint32_t mask = 0x80808080u - nib01(b16, n);
            fl[rt][n] = (int)(mask & lw4[n]);
            fh[rt][n] = (int)(mask & hw4[n]);
          }
        }
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const uint32_t b16 = ((m < 2 ? kv[ct].x : kv[ct].y) >> (16 * (m & 1))) & 0xFFFFu;
#pragma unroll
          for (int n = 0; n < 4; ++n) fb[ct][n] = (int)nib01(b16, n);
        }
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) {
            alo[rt][ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fl[rt], fb[ct], alo[rt][ct], 0, 0, 0);
            ahi[rt][ct] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fh[rt], fb[ct], ahi[rt][ct], 0, 0, 0);
          }
      }
    }
    __syncthreads();
  }

  // C/D of the 16 x 16 tile: column (key) = lane & 15, row (query) = 4 (lane >> 4) + register
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int lr = wq + 16 * rt + 4 * g + e, t = q0 + lr;
      if (t >= a.nq) continue;
      const int qr = qrow[lr];
      const double rs = qr >= 0 && a.row_scale ? a.row_scale[qr] : 1.0;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int lc = wk + 16 * ct + r, j = j0 + lc;
        if (j >= a.n_items) continue;
        float wgt;
        long long s;
        bool excl;
        if (qr < 0) {
          wgt = __uint_as_float(0x7FC00000u);
          s = -1;
          excl = true;
        } else {
          s = (long long)ahi[rt][ct][e] * 128 + (long long)alo[rt][ct][e];
          wgt = s ? wcooc_weight(s, rs, a.col_scale ? a.col_scale[j] : 1.0) : 0.0f;
          excl = s == 0 || j == qr;
        }
        const size_t o = (size_t)t * (size_t)a.n_items + (size_t)j;
        a.out_w[o] = wgt;
        if (a.out_sum) a.out_sum[o] = s;
        if (excl) atomicOr(&ex[lr][lc >> 5], 1u << (lc & 31));
      }
    }
  if (!a.out_excl) return;
  __syncthreads();
  if (tid < 2 * kWTile) {
    const int lr = tid >> 1, h = tid & 1, t = q0 + lr, wd = (j0 >> 5) + h;
    if (t < a.nq && wd < a.ewords) a.out_excl[(size_t)t * (size_t)a.ewords + wd] = ex[lr][h];
  }
}

static size_t wcooc_pad_users(int32_t n_users) {
  return ((size_t)n_users + kWChunkUsers - 1) / kWChunkUsers * kWChunkUsers;
}
static bool wcooc_aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace anirec

using namespace anirec;

extern "C" {

size_t anirec_wcooc_chunk_words(void) { return (size_t)kWChunk; }

size_t anirec_wcooc_workspace_bytes(int32_t n_items, int32_t n_users, int32_t nq) {
  if (n_items < 1 || n_users < 1 || n_users > kWMaxUsers || nq < 0) return 0;
  return 2 * wcooc_pad_users(n_users);
}

int anirec_wcooc_scores(const uint32_t *item_bits, int32_t n_items, int32_t n_users, const int32_t *user_q,
                        const int32_t *queries, int32_t nq, const double *row_scale, const double *col_scale,
                        float *out_w, int64_t *out_sum, uint32_t *out_excl, int32_t *err_flag, void *ws, size_t ws_bytes,
                        void *stream) {
  if (n_items < 1 || n_users < 1 || n_users > kWMaxUsers || nq < 0) return ANIREC_EINVAL;
  if (nq == 0) return ANIREC_OK;
  if (!item_bits || !user_q || !queries || !out_w || !err_flag || !ws) return ANIREC_EINVAL;
  if (!wcooc_aligned(item_bits, 4) || !wcooc_aligned(user_q, 4) || !wcooc_aligned(queries, 4) ||
      !wcooc_aligned(row_scale, 8) || !wcooc_aligned(col_scale, 8) || !wcooc_aligned(out_w, 4) ||
      !wcooc_aligned(out_sum, 8) || !wcooc_aligned(out_excl, 4) || !wcooc_aligned(err_flag, 4) || !wcooc_aligned(ws, 16))
    return ANIREC_EINVAL;
  const size_t pad = wcooc_pad_users(n_users);
  if (ws_bytes < 2 * pad) return ANIREC_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  WCoocArgs a;
  a.bits = item_bits;
  a.n_items = n_items;
  a.W = (n_users + 31) / 32;
  a.last_mask = (n_users & 31) ? (1u << (n_users & 31)) - 1u : 0xFFFFFFFFu;
  a.queries = queries;
  a.nq = nq;
  a.lo = (const uint32_t *)ws;
  a.hi = (const uint32_t *)((const char *)ws + pad);
  a.row_scale = row_scale;
  a.col_scale = col_scale;
  a.out_w = out_w;
  a.out_sum = (long long *)out_sum;
  a.out_excl = out_excl;
  a.ewords = (n_items + 31) / 32;
  a.err = err_flag;
  hipLaunchKernelGGL(k_wcooc_split, dim3((unsigned)((pad / 4 + 255) / 256)), dim3(256), 0, s, user_q, n_users, (int)pad,
                     (uint32_t *)ws, (uint32_t *)((char *)ws + pad), err_flag);
  const unsigned qt = ((unsigned)nq + kWTile - 1) / kWTile;
  const unsigned kt = ((unsigned)n_items + kWTile - 1) / kWTile;
  for (unsigned y0 = 0; y0 < qt; y0 += 32768u) {  // grid.y holds 65535 at the most
    WCoocArgs b = a;
    const unsigned ny = qt - y0 < 32768u ? qt - y0 : 32768u;
    const size_t t0 = (size_t)y0 * kWTile;
    b.queries = a.queries + t0;
    b.nq = (int)((size_t)nq - t0 < (size_t)ny * kWTile ? (size_t)nq - t0 : (size_t)ny * kWTile);
    b.out_w = a.out_w + t0 * (size_t)n_items;
    if (a.out_sum) b.out_sum = a.out_sum + t0 * (size_t)n_items;
    if (a.out_excl) b.out_excl = a.out_excl + t0 * (size_t)a.ewords;
    hipLaunchKernelGGL(k_wcooc, dim3(kt, ny), dim3(256), 0, s, b);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
