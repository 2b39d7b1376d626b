// Fold-in of new users for gfx950 (MI355X): fit one fresh user-embedding row per new user to that user's own ratings,
// every other layer of the model frozen (include/anirec.h, anirec_fold_in).
//
// The Keras model of neural_network.py:66-106 with the anime table, Dense(1) and BatchNorm (inference mode) frozen;
// model.fit full-batch on the user's n ratings with Keras-2.12 Adam, `steps` iterations.  The fits of different users
// share nothing but the frozen table, so a call is
//   pre-pass   Ah = l2-normalised anime rows into the workspace, once (rownorm_body<1>, the train step's forward form)
//   k_fold_in  one workgroup of 256 lanes per user, every step inside the one launch.  A row is one float4 per lane of a
//              group of kG = width / 4 lanes; the workgroup holds kNG = 256 / kG groups (32, 16, 8, 4 at widths 32, 64,
//              128, 256).  EVERY group keeps the user's u, m, v in registers (identical copies).  Per step, group g walks
//              ratings g, g + kNG, ... of the list in that order: gathers Ah[a_i], the cosine by the group butterfly, the
//              head, and adds dc_i (ah_i - c_i uh) to its float4 accumulator.  The kNG partial rows and loss sums meet in
//              LDS: every lane adds the kNG values of its column in group order 0 .. kNG-1, so all groups hold the same
//              gradient and take the same Adam step.  No atomics; the order depends on nothing but the user's own list:
//              a user's result is the same bits run to run, alone or in any batch, at any position.
// LDS: 256 float4 + kNG floats (4.1 KB at most) per workgroup; the Ah rows are not staged (they come through L2: a
// 17 560 x 128 table is 9 MB), so a list of any length takes the one path.
// The second half of the file is the same fit for a few rows with long lists (new anime against the user table,
// anirec_fold_in_split): the list split into chunks across workgroups, two launches per step.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "anirec_dev.hpp"

namespace anirec {

struct FoldArgs {
  const float *Ah;          // [n_anime][dim] normalised anime rows (workspace)
  int n_anime;
  const int64_t *offsets;   // [n_new + 1]
  const int32_t *anime_idx;
  const float *rating;
  const float *init;        // [n_new][dim]
  const float *alpha;       // [steps]
  int steps;
  float hs, hb, l2;
  int act, loss;
  float *out_rows;          // [n_new][dim]
  float *out_loss;          // [n_new]
  int32_t *err;
};

// one rating through the head chosen at run time: p, dl/dy and the data loss by head_grad / head_loss of that pair
// (the switch is uniform over the launch)
__device__ __forceinline__ void head_any(int act, int loss, float y, float t, float &g, float &l) {
  float p;
#define ANIREC_FOLD_CASE(A, L)                    \
  case (A)*8 + (L):                               \
    head_grad<(A), (L)>(y, t, p, g);              \
    l = head_loss<(A), (L)>(y, t, p);             \
    break;
#define ANIREC_FOLD_ACT(A)                                                                   \
  ANIREC_FOLD_CASE(A, ANIREC_LOSS_BCE) ANIREC_FOLD_CASE(A, ANIREC_LOSS_MSE)                  \
  ANIREC_FOLD_CASE(A, ANIREC_LOSS_MAE) ANIREC_FOLD_CASE(A, ANIREC_LOSS_HUBER)                \
  ANIREC_FOLD_CASE(A, ANIREC_LOSS_LOGCOSH)
  switch (act * 8 + loss) {
    ANIREC_FOLD_ACT(ANIREC_ACT_LINEAR)
    ANIREC_FOLD_ACT(ANIREC_ACT_TANH)
    ANIREC_FOLD_ACT(ANIREC_ACT_RELU)
    ANIREC_FOLD_ACT(ANIREC_ACT_SOFTPLUS)
    ANIREC_FOLD_CASE(ANIREC_ACT_SIGMOID, ANIREC_LOSS_MSE)
    ANIREC_FOLD_CASE(ANIREC_ACT_SIGMOID, ANIREC_LOSS_MAE)
    ANIREC_FOLD_CASE(ANIREC_ACT_SIGMOID, ANIREC_LOSS_HUBER)
    ANIREC_FOLD_CASE(ANIREC_ACT_SIGMOID, ANIREC_LOSS_LOGCOSH)
    default:
      head_grad<ANIREC_ACT_SIGMOID, ANIREC_LOSS_BCE>(y, t, p, g);
      l = head_loss<ANIREC_ACT_SIGMOID, ANIREC_LOSS_BCE>(y, t, p);
      break;
  }
#undef ANIREC_FOLD_ACT
#undef ANIREC_FOLD_CASE
}

template <int kD>
__global__ __launch_bounds__(256) void k_fold_in(FoldArgs a) {
#pragma clang fp contract(off)
  constexpr int kG = kD / 4, kNG = 256 / kG;
  __shared__ __attribute__((aligned(16))) float4 red[256];  // [kNG][kG]: the groups' partial gradient rows
  __shared__ float lred[kNG];                               // the groups' partial loss sums
  const int tid = threadIdx.x, l = tid & (kG - 1), g = tid / kG;
  const size_t u = blockIdx.x;
  float4 *out4 = reinterpret_cast<float4 *>(a.out_rows) + u * kG;
  const float4 w0 = reinterpret_cast<const float4 *>(a.init)[u * kG + l];
  const float qnan = __uint_as_float(0x7FC00000u);
  const long long lo = a.offsets[u], hi = a.offsets[u + 1];
  const bool bad_range = lo < 0 || hi < lo || hi - lo > (long long)INT_MAX;
  if (!bad_range && hi == lo) {  // no ratings: the start row bit for bit, no loss to report
    if (g == 0) out4[l] = w0;
    if (tid == 0) a.out_loss[u] = qnan;
    return;
  }
  // nothing is read through a bad offset pair or a bad index: the whole list is checked before any row is gathered
  const int n = bad_range ? 0 : (int)(hi - lo);
  const int32_t *ai = a.anime_idx + (bad_range ? 0 : lo);
  const float *rt = a.rating + (bad_range ? 0 : lo);
  int bad = bad_range ? 1 : 0;
  for (int i = tid; i < n; i += 256) bad |= ((uint32_t)ai[i] >= (uint32_t)a.n_anime) ? 1 : 0;
  if (__syncthreads_or(bad)) {
    if (g == 0) out4[l] = make_float4(qnan, qnan, qnan, qnan);
    if (tid == 0) {
      a.out_loss[u] = qnan;
      *a.err = 1;
    }
    return;
  }
  const float4 *Ah4 = reinterpret_cast<const float4 *>(a.Ah);
  const float nf = (float)n, two_l2 = 2.0f * a.l2;
  float4 w = w0;
  float4 m = make_float4(0.f, 0.f, 0.f, 0.f), v = m;
  for (int s = 0;; ++s) {
    const float ss = group_sum<kG>(w.x * w.x + w.y * w.y + w.z * w.z + w.w * w.w);
    const float ru = 1.0f / sqrtf(fmaxf(ss, kL2nEps));
    const float4 uh = make_float4(w.x * ru, w.y * ru, w.z * ru, w.w * ru);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float lsum = 0.f;
    for (int i = g; i < n; i += kNG) {
      const float4 x = Ah4[(size_t)ai[i] * kG + l];
      const float t = rt[i];
      const float c = group_sum<kG>(uh.x * x.x + uh.y * x.y + uh.z * x.z + uh.w * x.w);
      const float y = __fmaf_rn(c, a.hs, a.hb);
      float gy, li;
      head_any(a.act, a.loss, y, t, gy, li);
      lsum += li;
      const float dc = (gy / nf) * a.hs;
      acc.x += dc * (x.x - c * uh.x);
      acc.y += dc * (x.y - c * uh.y);
      acc.z += dc * (x.z - c * uh.z);
      acc.w += dc * (x.w - c * uh.w);
    }
    red[tid] = acc;
    if (l == 0) lred[g] = lsum;
    __syncthreads();
    float4 gs = red[l];
    float lt = lred[0];
#pragma unroll 4
    for (int k = 1; k < kNG; ++k) {  // fixed order: group 0, 1, ..., the same in every group
      const float4 q = red[k * kG + l];
      gs.x += q.x;
      gs.y += q.y;
      gs.z += q.z;
      gs.w += q.w;
      lt += lred[k];
    }
    __syncthreads();  // red / lred are rewritten by the next step
    if (s >= a.steps) {  // the loss at the row the last step left
      if (g == 0) out4[l] = w;
      if (tid == 0) a.out_loss[u] = lt / nf + a.l2 * ss;
      return;
    }
    const float al = a.alpha[s];
    adam_elem(w.x, m.x, v.x, ru * gs.x + two_l2 * w.x, al);
    adam_elem(w.y, m.y, v.y, ru * gs.y + two_l2 * w.y, al);
    adam_elem(w.z, m.z, v.z, ru * gs.z + two_l2 * w.z, al);
    adam_elem(w.w, m.w, v.w, ru * gs.w + two_l2 * w.w, al);
  }
}

static size_t fold_bytes(int32_t n_anime, int32_t dim) { return (size_t)n_anime * (size_t)dim * sizeof(float); }

// ---- the same fit with a row's list split across workgroups (anirec_fold_in_split) ----------------------------------
// A few dozen rows with lists of 10^3 .. 10^5 ratings (new anime against the user table): one workgroup per row would
// leave most of the chip idle and walk each list serially.  Here a list is cut into chunks of kChunk ratings and a
// step is two plain launches on the stream:
//   k_fold_part  one workgroup per chunk: k_fold_in's walk over the chunk's ratings (group g takes ratings g, g + kNG,
//                ... OF THE CHUNK), the kNG partial rows and loss sums added in LDS in group order, one partial row and
//                one partial loss stored into the chunk's slot
//   k_fold_step  one lane group per row: the row's partials added in ascending chunk order, starting from chunk 0's
//                value, then k_fold_in's gradient and Adam step on u (out_rows), m, v (workspace) in place
// after k_fold_check (every offsets pair, index and the chunk map validated; u = init, m = v = 0) and before
// k_fold_part once more + k_fold_final (the loss at the final row).  The kernel boundary is the only ordering between
// the two halves of a step: no grid-wide wait, no cooperative launch, no atomics.  A list of at most kChunk ratings is
// one chunk, and every operation on it is k_fold_in's: the same bits.
constexpr int kChunk = ANIREC_FOLD_CHUNK;

struct SplitArgs {
  const float *Th;          // [n_table][dim] normalised table rows (workspace)
  int n_table, n_new, n_chunks, dim;
  const int64_t *offsets;   // [n_new + 1]
  const int32_t *idx;
  const float *rating;
  const int32_t *chunk_offsets;  // [n_new + 1]
  const int32_t *chunk_row;      // [n_chunks]
  const float *init;        // [n_new][dim]
  const float *alpha;       // [steps]
  float hs, hb, l2;
  int act, loss;
  float *out_rows;          // [n_new][dim]: the rows being fitted live here between the launches
  float *out_loss;          // [n_new]
  int32_t *err;
  float *m, *v;             // [n_new][dim] (workspace)
  float *part;              // [n_chunks][dim] partial gradient rows (workspace)
  float *part_loss;         // [n_chunks] (workspace)
  int32_t *bad;             // [n_new] row flags, then one word: the chunk map is not the offsets' (workspace, zeroed)
};

// the number of ratings of a row, 0 for a bad pair; `bad` says which
__device__ __forceinline__ int fold_list_len(long long lo, long long hi, bool &bad) {
  bad = lo < 0 || hi < lo || hi - lo > (long long)INT_MAX;
  return bad ? 0 : (int)(hi - lo);
}

// grid (n_new, kCheckY): block (r, y) checks ratings y*256 + tid, + 256*kCheckY, ... of row r; block (r, 0) checks the
// row's offsets pair and chunk count and writes the start state; the chunk_row entries are spread over all threads.
// Every flag store writes the value 1 into a zeroed word.
constexpr int kCheckY = 16;
__global__ __launch_bounds__(256) void k_fold_check(SplitArgs a) {
  const int tid = threadIdx.x, r = blockIdx.x, y = blockIdx.y;
  int32_t *map_bad = a.bad + a.n_new;
  bool bad_range;
  const long long lo = a.offsets[r];
  const int n = fold_list_len(lo, a.offsets[r + 1], bad_range);
  int bad = 0;
  for (long long i = (long long)y * 256 + tid; i < n; i += 256 * kCheckY)
    bad |= ((uint32_t)a.idx[lo + i] >= (uint32_t)a.n_table) ? 1 : 0;
  if (y == 0) {
    if (tid == 0) {
      if (bad_range) bad = 1;
      const int c0 = a.chunk_offsets[r], c1 = a.chunk_offsets[r + 1];
      bool wrong = (long long)c1 - c0 != ((long long)n + kChunk - 1) / kChunk;
      if (r == 0 && c0 != 0) wrong = true;
      if (r == a.n_new - 1 && c1 != a.n_chunks) wrong = true;
      if (wrong) *map_bad = 1;
    }
    const int kg = a.dim / 4;
    if (tid < kg) {
      const size_t at = (size_t)r * kg + tid;
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      reinterpret_cast<float4 *>(a.out_rows)[at] = reinterpret_cast<const float4 *>(a.init)[at];
      reinterpret_cast<float4 *>(a.m)[at] = z;
      reinterpret_cast<float4 *>(a.v)[at] = z;
    }
  }
  if (bad) a.bad[r] = 1;
  // chunk c belongs to row q = chunk_row[c] iff chunk_offsets[q] <= c < chunk_offsets[q + 1]; with every row's count
  // right (above) that makes the map the one the offsets define
  const long long total = (long long)gridDim.x * gridDim.y * 256;
  for (long long c = ((long long)y * gridDim.x + r) * 256 + tid; c < a.n_chunks; c += total) {
    const int32_t q = a.chunk_row[c];
    if ((uint32_t)q >= (uint32_t)a.n_new || c < a.chunk_offsets[q] || c >= a.chunk_offsets[q + 1]) *map_bad = 1;
  }
}

template <int kD>
__global__ __launch_bounds__(256) void k_fold_part(SplitArgs a) {
#pragma clang fp contract(off)
  constexpr int kG = kD / 4, kNG = 256 / kG;
  __shared__ __attribute__((aligned(16))) float4 red[256];  // [kNG][kG]: the groups' partial gradient rows
  __shared__ float lred[kNG];                               // the groups' partial loss sums
  const int tid = threadIdx.x, l = tid & (kG - 1), g = tid / kG;
  const int c = blockIdx.x;
  if (a.bad[a.n_new]) return;  // nothing is read through a bad chunk map
  const int r = a.chunk_row[c];
  if (a.bad[r]) return;        // nor through a bad offsets pair or index
  const long long lo = a.offsets[r];
  const int n = (int)(a.offsets[r + 1] - lo);
  const int first = (c - a.chunk_offsets[r]) * kChunk;
  const int cnt = min(kChunk, n - first);
  const int32_t *ai = a.idx + lo + first;
  const float *rt = a.rating + lo + first;
  const float4 *Th4 = reinterpret_cast<const float4 *>(a.Th);
  const float nf = (float)n;
  const float4 w = reinterpret_cast<const float4 *>(a.out_rows)[(size_t)r * kG + l];
  const float ss = group_sum<kG>(w.x * w.x + w.y * w.y + w.z * w.z + w.w * w.w);
  const float ru = 1.0f / sqrtf(fmaxf(ss, kL2nEps));
  const float4 uh = make_float4(w.x * ru, w.y * ru, w.z * ru, w.w * ru);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float lsum = 0.f;
  for (int i = g; i < cnt; i += kNG) {
    const float4 x = Th4[(size_t)ai[i] * kG + l];
    const float t = rt[i];
    const float cs = group_sum<kG>(uh.x * x.x + uh.y * x.y + uh.z * x.z + uh.w * x.w);
    const float y = __fmaf_rn(cs, a.hs, a.hb);
    float gy, li;
    head_any(a.act, a.loss, y, t, gy, li);
    lsum += li;
    const float dc = (gy / nf) * a.hs;
    acc.x += dc * (x.x - cs * uh.x);
    acc.y += dc * (x.y - cs * uh.y);
    acc.z += dc * (x.z - cs * uh.z);
    acc.w += dc * (x.w - cs * uh.w);
  }
  red[tid] = acc;
  if (l == 0) lred[g] = lsum;
  __syncthreads();
  if (g != 0) return;
  float4 gs = red[l];
  float lt = lred[0];
#pragma unroll 4
  for (int k = 1; k < kNG; ++k) {  // fixed order: group 0, 1, ...
    const float4 q = red[k * kG + l];
    gs.x += q.x;
    gs.y += q.y;
    gs.z += q.z;
    gs.w += q.w;
    lt += lred[k];
  }
  reinterpret_cast<float4 *>(a.part)[(size_t)c * kG + l] = gs;
  if (l == 0) a.part_loss[c] = lt;
}

// One lane group per row, kNG rows per workgroup.  kFinal: the loss at the row instead of a step.
template <int kD, bool kFinal>
__global__ __launch_bounds__(256) void k_fold_step(SplitArgs a, int s) {
#pragma clang fp contract(off)
  constexpr int kG = kD / 4, kNG = 256 / kG;
  const int tid = threadIdx.x, l = tid & (kG - 1), g = tid / kG;
  const int row = blockIdx.x * kNG + g;
  const bool live = row < a.n_new;
  const int r = live ? row : 0;
  float4 *u4 = reinterpret_cast<float4 *>(a.out_rows) + (size_t)r * kG + l;
  float4 w = *u4;
  const float ss = group_sum<kG>(w.x * w.x + w.y * w.y + w.z * w.z + w.w * w.w);  // before any group leaves
  if (!live) return;
  const float qnan = __uint_as_float(0x7FC00000u);
  if (a.bad[a.n_new] || a.bad[r]) {  // the row and its loss become NaN at the end; nothing is read through the fault
    if (kFinal) {
      *u4 = make_float4(qnan, qnan, qnan, qnan);
      if (l == 0) {
        a.out_loss[r] = qnan;
        *a.err = 1;
      }
    }
    return;
  }
  const int n = (int)(a.offsets[r + 1] - a.offsets[r]);
  if (n == 0) {  // no ratings: the start row stays, no loss to report
    if (kFinal && l == 0) a.out_loss[r] = qnan;
    return;
  }
  const int c0 = a.chunk_offsets[r], c1 = a.chunk_offsets[r + 1];
  const float nf = (float)n;
  if (kFinal) {
    float lt = a.part_loss[c0];
    for (int c = c0 + 1; c < c1; ++c) lt += a.part_loss[c];
    if (l == 0) a.out_loss[r] = lt / nf + a.l2 * ss;
    return;
  }
  const float4 *p4 = reinterpret_cast<const float4 *>(a.part);
  float4 gs = p4[(size_t)c0 * kG + l];
  for (int c = c0 + 1; c < c1; ++c) {  // fixed order: chunk 0, 1, ...
    const float4 q = p4[(size_t)c * kG + l];
    gs.x += q.x;
    gs.y += q.y;
    gs.z += q.z;
    gs.w += q.w;
  }
  const float ru = 1.0f / sqrtf(fmaxf(ss, kL2nEps));
  const float two_l2 = 2.0f * a.l2;
  float4 *m4 = reinterpret_cast<float4 *>(a.m) + (size_t)r * kG + l;
  float4 *v4 = reinterpret_cast<float4 *>(a.v) + (size_t)r * kG + l;
  float4 m = *m4, v = *v4;
  const float al = a.alpha[s];
  adam_elem(w.x, m.x, v.x, ru * gs.x + two_l2 * w.x, al);
  adam_elem(w.y, m.y, v.y, ru * gs.y + two_l2 * w.y, al);
  adam_elem(w.z, m.z, v.z, ru * gs.z + two_l2 * w.z, al);
  adam_elem(w.w, m.w, v.w, ru * gs.w + two_l2 * w.w, al);
  *u4 = w;
  *m4 = m;
  *v4 = v;
}

static size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

// workspace: Th [n_table][dim] | m [n_new][dim] | v [n_new][dim] | part [n_chunks][dim] | part_loss [n_chunks] |
// bad [n_new + 1], each part at a multiple of 16 bytes
struct SplitLayout {
  size_t m, v, part, part_loss, bad, total;
};
static SplitLayout split_layout(int32_t n_table, int32_t n_new, int32_t n_chunks, int32_t dim) {
  const size_t row = (size_t)dim * sizeof(float);
  SplitLayout o;
  o.m = (size_t)n_table * row;
  o.v = o.m + (size_t)n_new * row;
  o.part = o.v + (size_t)n_new * row;
  o.part_loss = o.part + (size_t)n_chunks * row;
  o.bad = o.part_loss + up16((size_t)n_chunks * sizeof(float));
  o.total = o.bad + up16(((size_t)n_new + 1) * sizeof(int32_t));
  return o;
}

}  // namespace anirec

using namespace anirec;

extern "C" {

size_t anirec_fold_in_workspace_bytes(int32_t n_anime, int32_t n_new, int32_t dim) {
  if (n_anime < 1 || n_new < 0 || !dim_ok(dim)) return 0;
  return fold_bytes(n_anime, dim);
}

int anirec_fold_in(const float *A, int32_t dim, int32_t n_anime, const anirec_head *head, int32_t activation,
                   int32_t loss, float l2, const int64_t *offsets, const int32_t *anime_idx, const float *rating,
                   int32_t n_new, const float *init, const float *alpha, int32_t steps, float *out_rows,
                   float *out_loss, int32_t *err_flag, void *workspace, size_t workspace_bytes, void *stream) {
  if (!dim_ok(dim) || !act_ok(activation) || !loss_ok(loss) || n_anime < 1 || n_new < 0 || steps < 0)
    return ANIREC_EINVAL;
  if (n_new == 0) return ANIREC_OK;
  if (!A || !head || !offsets || !init || !out_rows || !out_loss || !err_flag || !workspace || (steps > 0 && !alpha))
    return ANIREC_EINVAL;
  if (workspace_bytes < fold_bytes(n_anime, dim)) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  float *Ah = (float *)workspace;
  l2norm_rows(A, n_anime, Ah, dim, s);
  ANIREC_HIP_CHECK(hipGetLastError());
  FoldArgs a;
  a.Ah = Ah;
  a.n_anime = n_anime;
  a.offsets = offsets;
  a.anime_idx = anime_idx;
  a.rating = rating;
  a.init = init;
  a.alpha = alpha;
  a.steps = steps;
  head_affine_f32(head, &a.hs, &a.hb);
  a.l2 = l2;
  a.act = activation;
  a.loss = loss;
  a.out_rows = out_rows;
  a.out_loss = out_loss;
  a.err = err_flag;
  with_width(dim, [&](auto kd) {
    hipLaunchKernelGGL(k_fold_in<decltype(kd)::value>, dim3((unsigned)n_new), dim3(256), 0, s, a);
  });
  return (int)hipGetLastError();
}

size_t anirec_fold_in_split_workspace_bytes(int32_t n_table, int32_t n_new, int32_t n_chunks, int32_t dim) {
  if (n_table < 1 || n_new < 0 || n_chunks < 0 || !dim_ok(dim)) return 0;
  return split_layout(n_table, n_new, n_chunks, dim).total;
}

int anirec_fold_in_split(const float *T, int32_t dim, int32_t n_table, const anirec_head *head, int32_t activation,
                         int32_t loss, float l2, const int64_t *offsets, const int32_t *idx, const float *rating,
                         int32_t n_new, const int32_t *chunk_offsets, const int32_t *chunk_row, int32_t n_chunks,
                         const float *init, const float *alpha, int32_t steps, float *out_rows, float *out_loss,
                         int32_t *err_flag, void *workspace, size_t workspace_bytes, void *stream) {
  if (!dim_ok(dim) || !act_ok(activation) || !loss_ok(loss) || n_table < 1 || n_new < 0 || n_chunks < 0 || steps < 0)
    return ANIREC_EINVAL;
  if (n_new == 0) return ANIREC_OK;
  if (!T || !head || !offsets || !chunk_offsets || !init || !out_rows || !out_loss || !err_flag || !workspace ||
      (steps > 0 && !alpha) || (n_chunks > 0 && !chunk_row))
    return ANIREC_EINVAL;
  const SplitLayout lay = split_layout(n_table, n_new, n_chunks, dim);
  if (workspace_bytes < lay.total) return ANIREC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  char *ws = (char *)workspace;
  SplitArgs a;
  a.bad = (int32_t *)(ws + lay.bad);
  ANIREC_HIP_CHECK(hipMemsetAsync(err_flag, 0, 4, s));
  ANIREC_HIP_CHECK(hipMemsetAsync(a.bad, 0, ((size_t)n_new + 1) * sizeof(int32_t), s));
  float *Th = (float *)workspace;
  l2norm_rows(T, n_table, Th, dim, s);
  ANIREC_HIP_CHECK(hipGetLastError());
  a.Th = Th;
  a.n_table = n_table;
  a.n_new = n_new;
  a.n_chunks = n_chunks;
  a.dim = dim;
  a.offsets = offsets;
  a.idx = idx;
  a.rating = rating;
  a.chunk_offsets = chunk_offsets;
  a.chunk_row = chunk_row;
  a.init = init;
  a.alpha = alpha;
  head_affine_f32(head, &a.hs, &a.hb);
  a.l2 = l2;
  a.act = activation;
  a.loss = loss;
  a.out_rows = out_rows;
  a.out_loss = out_loss;
  a.err = err_flag;
  a.m = (float *)(ws + lay.m);
  a.v = (float *)(ws + lay.v);
  a.part = (float *)(ws + lay.part);
  a.part_loss = (float *)(ws + lay.part_loss);
  hipLaunchKernelGGL(k_fold_check, dim3((unsigned)n_new, kCheckY), dim3(256), 0, s, a);
  with_width(dim, [&](auto kd) {
    constexpr int kD = decltype(kd)::value;
    const dim3 rows((unsigned)((n_new + 1024 / kD - 1) / (1024 / kD)));  // 256 / (kD / 4) rows per workgroup
    for (int st = 0; st <= steps; ++st) {
      if (n_chunks > 0) hipLaunchKernelGGL(k_fold_part<kD>, dim3((unsigned)n_chunks), dim3(256), 0, s, a);
      if (st < steps)
        hipLaunchKernelGGL((k_fold_step<kD, false>), rows, dim3(256), 0, s, a, st);
      else
        hipLaunchKernelGGL((k_fold_step<kD, true>), rows, dim3(256), 0, s, a, st);
    }
  });
  return (int)hipGetLastError();
}

}  // extern "C"
