// The lazy dense Adam's replay of a row's pending L2-only steps (include/anirec.h, "LAZY DENSE ADAM"), inlined into
// the kernels of four units: the lazy kernels and the whole-replay self-test (anirec_train.hip), the two head kernels,
// whose launches carry a share of the catch-up (anirec_train_head.hip, anirec_train_head_metrics.hip), and the self-tests
// of the square root and the divide (anirec_train_util.hip).  Each of the first three gets its own copy of the
// out-of-line slow path, lazy_replay_slow.
#pragma once
#include "anirec_train.hpp"

namespace anirec {

struct Row3 {
  float4 w, m, v;
};

// pending pure-L2 steps [j0, j1) (window-relative) of one row, a float4 per lane: g = 2 lambda W exactly as the
// dense kernel forms it for a row no rating touched; sq[j] receives this lane's part of sum(W_s^2), the weights
// step s READ
// the dense kernel's gradient of a row no rating touched, grad_total(0, 0, w, 2 lambda) = (0 - 0 w) + 2 lambda w:
// (0 - 0 w) is +0 for every finite w, so it is (2 lambda w) + 0 — the "+ 0" kept because it turns a -0 product into
// the +0 the dense expression yields (bit-identical tables, zeros included)
__device__ __forceinline__ float l2_only_grad(float w, float two_l2) {
#pragma clang fp contract(off)
  return two_l2 * w + 0.0f;
}

// ---- the replayed Adam step on packed pairs -----------------------------------------------------------------
// The flush is bound by its arithmetic: the compiler's correctly rounded sqrtf (15 instructions: scaling for tiny
// inputs, v_sqrt_f32, two +-1 ulp residual tests, class fix-up) and IEEE divide (11: v_div_scale x2, v_rcp_f32, the
// Markstein fma chain, v_div_fmas, v_div_fixup) per element-step, all scalar.  For operands in the exponent range
// Adam's moments live in, the scaling and fix-up steps are identities, and what is left — the residual tests and the
// fma chain, instruction for instruction what the expansions execute — runs on PAIRS (v_pk_fma_f32 / v_pk_mul_f32 /
// v_pk_add_f32).  A wave whose operands leave the range (a moment decayed to a denormal, an exact zero) takes the
// compiler's path for that row: the results are the dense kernel's bit for bit either way (tested on every element
// of the S109M tables; the square root is compared with sqrtf on EVERY float of its range, anirec_selftest_lazy_math).
//
// Round 4 (PMC: the kernel issues, it does not wait — profiles/r04_pmc_valu_train_s109m.json):
//  * the range tests left the step: every pair-step folds its second moment and |m alpha| into a running
//    min / max (v_min3_f32 / v_max3_f32: 4 instructions instead of 8 compares + 7 s_and) and the row is tested ONCE,
//    after its last step.  A NaN slips through min / max, but it is sticky (w NaN -> g, m, v NaN; m or v NaN -> w NaN),
//    so one test of the final w catches it.
//  * the square root is ONE exact-residual Newton correction from v_rsq_f32 (sqrt4_normal) instead of v_sqrt_f32
//    + both neighbours' residuals + a three-way selection (v_cmp + v_cndmask through VCC cost two wait states each
//    on gfx950 that the compiler could only half fill: 494 s_nop in the round-3 kernel).
//  * g = 2 lambda w without the "+ 0" of l2_only_grad: it only matters when the product is -0, and then the first
//    moment of that step is +-0, |m alpha| = 0 fails the range test and the row is redone by the compiler's path.
// Round 5: the running minima / maxima left the step too — the bounds are derived once per row from the values the
// replay starts from (lz_entry_ok), only the smallest |m| is still folded per step; and the divide takes one
// correction instead of two (div4_normal, checked by exhaustion).
// The four elements of a lane are two PAIRS stepped side by side, statement by statement: every operation is two
// independent v_pk_*_f32 back to back.  (Written as one pair after the other, hipcc ran one pair's divide chain behind
// the other's — gfx950 wants a wait state between DEPENDENT packed-f32 instructions, and that schedule paid an s_nop
// for each; written as one 4-wide vector, its subtractions and negations come out scalar.)
typedef float f32x2 __attribute__((ext_vector_type(2)));
struct Quad {
  f32x2 a, b;
};
// (the contraction flag of an operation is the one in force where it is WRITTEN: these bodies, not their callers)
#pragma clang fp contract(off)
__device__ __forceinline__ Quad operator+(Quad x, Quad y) { return {x.a + y.a, x.b + y.b}; }
__device__ __forceinline__ Quad operator-(Quad x, Quad y) { return {x.a - y.a, x.b - y.b}; }
__device__ __forceinline__ Quad operator*(Quad x, Quad y) { return {x.a * y.a, x.b * y.b}; }
__device__ __forceinline__ Quad operator*(Quad x, float y) { return {x.a * y, x.b * y}; }
__device__ __forceinline__ Quad operator+(Quad x, float y) { return {x.a + y, x.b + y}; }
__device__ __forceinline__ Quad operator-(Quad x) { return {-x.a, -x.b}; }
#pragma clang fp contract(fast)
__device__ __forceinline__ Quad qfma(Quad x, Quad y, Quad z) {
  return {__builtin_elementwise_fma(x.a, y.a, z.a), __builtin_elementwise_fma(x.b, y.b, z.b)};
}

// Correctly rounded sqrt of x in [2^-96, 2^96] (no scaling of tiny inputs needed there): y = v_rsq_f32(x),
// s0 = x y, h = y / 2, then ONE Newton correction with the EXACT residual (fma): s = s0 + (x - s0^2) h.
// 4 packed operations + 1 transcendental per element, against 1 + 9 for the form the compiler expands sqrtf into
// (v_sqrt_f32, both neighbours' residuals, a three-way selection).  In general such a step is only faithful: that on
// gfx950 — with this part's v_rsq_f32 — its fma rounds to the correctly rounded root for EVERY float of the range is
// not argued but CHECKED: anirec_selftest_lazy_math compares it with sqrtf on all 1.6e9 of them
// (tests/test_train_gpu.py: 0 mismatches; the same code without the correction, kSteps = 0, misses on 4.8e8 — the
// comparison can fail; with a second correction, kSteps = 2, measured 0 as well and 7 % slower).  A part whose
// transcendental unit rounded differently would fail that test, not silently change a table.
template <int kSteps = 1>
__device__ __forceinline__ Quad sqrt4_normal(Quad x) {
#pragma clang fp contract(off)
  Quad y;
  y.a.x = __builtin_amdgcn_rsqf(x.a.x);
  y.a.y = __builtin_amdgcn_rsqf(x.a.y);
  y.b.x = __builtin_amdgcn_rsqf(x.b.x);
  y.b.y = __builtin_amdgcn_rsqf(x.b.y);
  const Quad s0 = x * y;
  if (kSteps == 0) return s0;
  const Quad h = y * 0.5f;
  const Quad d0 = qfma(-s0, s0, x);
  const Quad s1 = qfma(d0, h, s0);
  if (kSteps == 1) return s1;
  const Quad d1 = qfma(-s1, s1, x);
  return qfma(d1, h, s1);
}

// refined reciprocal y = y0 + (1 - d y0) y0, y0 = v_rcp_f32(d): anirec_selftest_lazy_div checks y == 1.0f / d on
// EVERY float d of [1e-7, 2^48] (the denominators sqrt(v) + 1e-7 the replay admits)
__device__ __forceinline__ Quad rcp4_refined(Quad d) {
#pragma clang fp contract(off)
  Quad y0;
  y0.a.x = __builtin_amdgcn_rcpf(d.a.x);
  y0.a.y = __builtin_amdgcn_rcpf(d.a.y);
  y0.b.x = __builtin_amdgcn_rcpf(d.b.x);
  y0.b.y = __builtin_amdgcn_rcpf(d.b.y);
  const Quad one = {{1.0f, 1.0f}, {1.0f, 1.0f}};
  const Quad e = qfma(-d, y0, one);
  return qfma(e, y0, y0);
}

// Correctly rounded n / d for |n| in [2^-60, 2^60], d in [1e-7, 2^48]: q0 = n y, ONE correction q1 = q0 + (n - d q0) y.
// The compiler's chain (v_div_scale / v_div_fixup aside) takes a second one, r1 = n - d q1, q2 = q1 + r1 y, because
// Markstein's theorem — y = RN(1/d), q within 1 ulp of n/d, the residual n - d q exact, no underflow — then makes q2
// = RN(n/d) for any q1 within 1 ulp.  It does NOT cover q1 itself: with y = RN(1/d), q0 = RN(n y) is off by up to
// 1.48 ulp and the fma's residual n - d q0 is inexact for ~0.15 % of operand pairs.  q1 = RN(n/d) is established by
// exhaustion instead (anirec_selftest_lazy_div, tests/test_lazy_div_exhaustive_gpu.py):
//  * y == RN(1/d) for every float d of the range (6e8 values), so y(d 2^k) = y(d) 2^k there;
//  * then every operation of the sequence commutes with scaling n and d by powers of two as long as no result is
//    subnormal: q0 and q1 are within 2 ulp of n/d in [2^-108, 2^84], and a nonzero residual n - d q0 is a multiple
//    of ulp(d) ulp(q0) >= 2^-48 |n| >= 2^-108 (normal: the fma rounds it once, as it does for n, d in [1, 2));
//  * so q1 == RN(n/d) for the whole range iff it holds for all 2^46 significand pairs n, d in [1, 2) (signs are
//    symmetric) — the self-test compares q1 with IEEE `/` on every one of them: 0 mismatches.
// (The second correction is 4 packed operations per lane-step, ~7 % of the flush's VALU issue.)
__device__ __forceinline__ Quad div4_normal(Quad n, Quad d) {
#pragma clang fp contract(off)
  const Quad y = rcp4_refined(d);
  const Quad q0 = n * y;
  const Quad r0 = qfma(-d, q0, n);
  return qfma(r0, y, q0);
}

// What the short sequences are exact for: every step's second moment in [2^-96, 2^96] (no sqrt scaling), |m alpha| in
// [2^-60, 2^60] with the denominator sqrt(v) + 1e-7 in [1e-7, 2^48 + eps] (no v_div_scale, no v_div_fixup).
// The bounds are tested ONCE per row, from the values the replay starts from, instead of folding every step's
// operands into running minima / maxima (round 4: 8 v_min3 / v_max3 per lane-step).  Window constants (lz_bound):
// amin / A = the smallest / largest alpha of the window's steps, L = |2 lambda|.  Per element, u = 2^-24, every
// operation rounding to nearest (monotone, |RN(x)| <= |x| (1 + u), and RN(x) >= x (1 - u) for normal x > 0; a flush
// to zero only lowers a magnitude), by induction over the <= 8 steps:
//  (v lo) g^2 >= 0, so RN(g^2 - v) >= RN(-v) = -v and v' = RN(v + RN(RN(g^2 - v) c2)) >= v (1 - c2 (1 + u)) (1 - u)
//         >= 0.99899 v for normal v.  The FIRST step also lifts v: with G = RN(g_0^2) normal, either v_0 <= G / 2,
//         then RN(G - v_0) >= (G - v_0) (1 - u) and v_1 >= (v_0 + (G - v_0) c2 (1 - u)^2) (1 - u) >= c2 G (1 - u)^3,
//         or v_0 > G / 2 and v_1 >= 0.99899 v_0 > c2 G.  So v_1 >= max(0.99899 v_0, c2 G (1 - u)^3), and the
//         per-element vb = max(v_0, e), e = RN(RN(c2 L^2) RN(w_0^2)) <= c2 G (1 - u)^-10, gives every v_j (j >= 1,
//         the moments the steps produce) >= 0.99899^7 (1 - 13 u) 0.99899 vb >= 0.989 vb > 2^-96 for vb >= 2^-95 (the
//         factor-2 margin).  (Rows fresh from initialisation, v_0 = 0, are admitted through e: |w_0| >~ 1e-9 at
//         lambda = 1e-4, as the per-step test of the moments admitted them.)
//  (v hi) v' is RN of a combination of v and RN(g^2) with weights (1 - c), c in (0, 1): v' <= max(v, g^2) (1 + u)^2.
//  (m)    likewise |m'| <= max(|m|, |g|) (1 + u)^3, and |g| = |RN(2 lambda w)| <= L |w| (1 + u).
//  (w)    |w'| <= (|w| + |q|) (1 + u), q = RN(RN(m' alpha) / RN(RN(sqrt v') + eps)), the denominator >= RN(sqrt v')
//         >= sqrt(0.989 vb) (1 - u) and >= eps: |q| <= |m'| S, S = min(1.006 A / sqrt(vb), 1.0001 A / eps) (the
//         second term is what bounds the first window's rows whose tiny |w_0| makes vb tiny).
//  With X = max(|m|, L |w|): X' <= X (1 + L S) (1 + u)^5.  Over the window, with F = (1 + L S)^8: every |m_j| and
//  |g_j| <= X_0 F (1 + 2^-17), so every v_j <= max(v_0, (X_0 F)^2) (1 + 2^-15) and |m_j alpha_j| <= A X_0 F (1 + 2^-16).
//  The row is admitted if every vb >= 2^-95, v_0 <= 2^95, X_0 F <= 2^46 and X_0 F A <= 2^58: a factor 2 below the
//  2^47 / 2^59 the bounds need, which covers F's own roundings in fp32 and v_rsq_f32's error (with 1.01 for 1.006
//  and for 1.0001; F is taken at the lane's smallest vb).
//  (|m alpha| lo) the one bound no entry value gives — m crossing zero — stays per step: the smallest |m_j| of the
//  steps taken (one v_min3 per pair), times amin once: RN(|m_j| alpha_j) >= RN(min |m| amin) >= 2^-60.
// A NaN slips through min / max (and fails every comparison); it is sticky (w NaN -> g, m, v NaN; m or v NaN -> w
// NaN), so the test of the final w catches it.
struct LzBound {
  float amin;  // smallest alpha of the window's steps [0, nj)
  float amax;  // A
  float k;     // 1.01 L A
  float kmax;  // 1.01 L A / eps
  float kv;    // c2 L^2
};
__device__ __forceinline__ LzBound lz_bound(const float (&alpha)[kLzWin], int nj, float two_l2) {
  float amin = 3.0e38f, amax = 0.f;
#pragma unroll
  for (int j = 0; j < kLzWin; ++j) {
    if (j < nj) amin = fminf(amin, alpha[j]);
    amax = fmaxf(amax, alpha[j]);
  }
  const float k = 1.01f * fabsf(two_l2) * amax;
  return {amin, amax, k, k * 1e7f, kOneMinusB2 * two_l2 * two_l2};
}
__device__ __forceinline__ float min3f(float a, float b, float c) { return fminf(fminf(a, b), c); }
__device__ __forceinline__ float max3f(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
// the entry half of the test above, for a lane's four elements
__device__ __forceinline__ bool lz_entry_ok(const Row3 &x, const LzBound &bd, float two_l2) {
  const float vb0 = fmaxf(x.v.x, bd.kv * (x.w.x * x.w.x)), vb1 = fmaxf(x.v.y, bd.kv * (x.w.y * x.w.y)),
              vb2 = fmaxf(x.v.z, bd.kv * (x.w.z * x.w.z)), vb3 = fmaxf(x.v.w, bd.kv * (x.w.w * x.w.w));
  const float vlo = fminf(min3f(vb0, vb1, vb2), vb3);
  const float vhi = fmaxf(max3f(x.v.x, x.v.y, x.v.z), x.v.w);
  const float mx = fmaxf(max3f(fabsf(x.m.x), fabsf(x.m.y), fabsf(x.m.z)), fabsf(x.m.w));
  const float wx = fmaxf(max3f(fabsf(x.w.x), fabsf(x.w.y), fabsf(x.w.z)), fabsf(x.w.w));
  const float x0 = fmaxf(mx, fabsf(two_l2) * wx);
  float f = 1.0f + fminf(bd.k * __builtin_amdgcn_rsqf(vlo), bd.kmax);
  f = f * f;
  f = f * f;
  f = f * f;
  const float xf = x0 * f;
  return vlo >= 0x1p-95f && vhi <= 0x1p95f && xf <= 0x1p46f && xf * bd.amax <= 0x1p58f;
}

// The catch-up (k_head / k_lazy_adam / k_lazy_catchup) replays a row's few pending steps on a latency-bound path:
// there the ~50 instructions of lz_bound + lz_entry_ok cost more than they save (measured: +0.3 / +0.75 / +0.35 us
// per launch), so it keeps the round-4 test instead — every pair-step folds its second moment and |m alpha| into
// running minima / maxima, tested after the row's last step (kRowTest = false).  The flush (a whole window per row,
// VALU-bound) takes the once-per-row test (kRowTest = true).
struct LzRange {
  float vlo, vhi, nlo, nhi;  // kRowTest: nlo = the smallest |m| alone
};
__device__ __forceinline__ bool lz_range_ok(const LzRange &r) {
  return r.vlo >= 0x1p-96f && r.vhi <= 0x1p96f && r.nlo >= 0x1p-60f && r.nhi <= 0x1p60f;
}

// one L2-only Adam step of a lane's four elements by the short sequences; kRowTest: the smallest |m| of the step is
// folded into rg.nlo (tested by the caller once per row, with the window's smallest alpha); otherwise every operand
// the sequences are conditional on is folded into rg
template <bool kRowTest>
__device__ __forceinline__ void adam4_l2(Quad &w, Quad &m, Quad &v, float alpha, float two_l2, LzRange &rg) {
#pragma clang fp contract(off)
  const Quad g = w * two_l2;
  const Quad mn = m + (g - m) * kOneMinusB1;
  const Quad vn = v + (g * g - v) * kOneMinusB2;
  const Quad num = mn * alpha;
  if (kRowTest) {
    rg.nlo = min3f(min3f(rg.nlo, fabsf(mn.a.x), fabsf(mn.a.y)), fabsf(mn.b.x), fabsf(mn.b.y));
  } else {
    rg.vlo = min3f(min3f(rg.vlo, vn.a.x, vn.a.y), vn.b.x, vn.b.y);
    rg.vhi = max3f(max3f(rg.vhi, vn.a.x, vn.a.y), vn.b.x, vn.b.y);
    rg.nlo = min3f(min3f(rg.nlo, fabsf(num.a.x), fabsf(num.a.y)), fabsf(num.b.x), fabsf(num.b.y));
    rg.nhi = max3f(max3f(rg.nhi, fabsf(num.a.x), fabsf(num.a.y)), fabsf(num.b.x), fabsf(num.b.y));
  }
  const Quad den = sqrt4_normal(vn) + kAdamEps;
  w = w - div4_normal(num, den);
  m = mn;
  v = vn;
}

template <bool kFast, bool kRowTest>
__device__ __forceinline__ void lazy_one_step(Row3 &x, float alpha, float two_l2, float &sq, LzRange &rg) {
  sq = x.w.x * x.w.x + x.w.y * x.w.y + x.w.z * x.w.z + x.w.w * x.w.w;
  if (kFast) {
    Quad w = {{x.w.x, x.w.y}, {x.w.z, x.w.w}}, m = {{x.m.x, x.m.y}, {x.m.z, x.m.w}}, v = {{x.v.x, x.v.y}, {x.v.z, x.v.w}};
    adam4_l2<kRowTest>(w, m, v, alpha, two_l2, rg);
    x.w = make_float4(w.a.x, w.a.y, w.b.x, w.b.y);
    x.m = make_float4(m.a.x, m.a.y, m.b.x, m.b.y);
    x.v = make_float4(v.a.x, v.a.y, v.b.x, v.b.y);
    return;
  }
  // the compiler's full expansions (scaling, fix-up)
  const float gx = l2_only_grad(x.w.x, two_l2), gy = l2_only_grad(x.w.y, two_l2), gz = l2_only_grad(x.w.z, two_l2),
              gw = l2_only_grad(x.w.w, two_l2);
  adam_elem(x.w.x, x.m.x, x.v.x, gx, alpha);
  adam_elem(x.w.y, x.m.y, x.v.y, gy, alpha);
  adam_elem(x.w.z, x.m.z, x.v.z, gz, alpha);
  adam_elem(x.w.w, x.m.w, x.v.w, gw, alpha);
}

// returns whether the short sequences were exact for every operand of every step this lane took (kFast)
template <bool kFast, bool kRowTest>
__device__ __forceinline__ bool lazy_replay_path(Row3 &x, int j0, int j1, const float (&alpha)[kLzWin], float two_l2,
                                                 const LzBound &bd, float (&sq)[kLzWin]) {
  const bool entry_ok = kFast && kRowTest ? lz_entry_ok(x, bd, two_l2) : true;
  LzRange rg = {3.0e38f, 0.f, 3.0e38f, 0.f};
  if (__all(j0 <= 0 && j1 >= kLzWin)) {  // the common case (a row untouched for a whole window): no predication
#pragma unroll
    for (int j = 0; j < kLzWin; ++j) lazy_one_step<kFast, kRowTest>(x, alpha[j], two_l2, sq[j], rg);
  } else {
#pragma unroll
    for (int j = 0; j < kLzWin; ++j) {
      if (__any(j >= j0 && j < j1)) {  // wave-uniform skip, then per-lane selection of the stepped values
        Row3 y = x;
        LzRange ry = rg;
        float q;
        lazy_one_step<kFast, kRowTest>(y, alpha[j], two_l2, q, ry);
        if (j >= j0 && j < j1) {
          x = y;
          rg = ry;
          sq[j] = q;
        }
      }
    }
  }
  if (!kFast) return true;
  if (j1 <= j0) return true;           // nothing taken
  const float t = (x.w.x + x.w.y) + (x.w.z + x.w.w);  // a NaN anywhere in the replay has reached w
  if (!kRowTest) return lz_range_ok(rg) && t == t;
  return entry_ok && rg.nlo * bd.amin >= 0x1p-60f && t == t;
}

// The replay by the compiler's full expansions, OUT OF LINE: it runs for a handful of rows per table (a moment decayed
// to a denormal, an exact zero) but, inlined, its 4 x 8 unrolled IEEE divides and square roots set the register
// allocation of every kernel that can reach it (the flush: 150-166 VGPRs, three waves per SIMD).  Everything goes in
// and out by value: an array whose address escaped into the call would live in scratch memory on the hot path too.
struct SlowReplay {
  Row3 x;
  float sq[kLzWin];
};
struct AlphaPack {
  float a[kLzWin];
};
__device__ __attribute__((noinline)) SlowReplay lazy_replay_slow(Row3 x, int j0, int j1, AlphaPack al, float two_l2) {
  SlowReplay o;
  float alpha[kLzWin], sq[kLzWin];
#pragma unroll
  for (int j = 0; j < kLzWin; ++j) {
    alpha[j] = al.a[j];
    sq[j] = 0.f;
  }
  (void)lazy_replay_path<false, false>(x, j0, j1, alpha, two_l2, LzBound{}, sq);
  o.x = x;
#pragma unroll
  for (int j = 0; j < kLzWin; ++j) o.sq[j] = sq[j];
  return o;
}

// pending pure-L2 steps [j0, j1) (window-relative) of one row, a float4 per lane; sq[j] receives this lane's part of
// sum(W_s^2), the weights step s READ, for the steps taken (the others keep what the caller put there).  The packed
// short sequences first; if any lane of the wave met an operand
// outside their range, the whole replay is redone from the saved row with the compiler's expansions (rare: a moment
// decayed to a denormal, an exact zero).
// (the row is re-read from memory for the redo — nothing has been stored yet — rather than kept in 12 more registers)
template <bool kRowTest>
__device__ __forceinline__ void lazy_replay(Row3 &x, int j0, int j1, const float (&alpha)[kLzWin], float two_l2,
                                            const LzBound &bd, float (&sq)[kLzWin], const float *W, const float *M,
                                            const float *V, size_t e) {
  if (__all(lazy_replay_path<true, kRowTest>(x, j0, j1, alpha, two_l2, bd, sq))) return;
  Row3 y;
  y.w = reinterpret_cast<const float4 *>(W)[e];
  y.m = reinterpret_cast<const float4 *>(M)[e];
  y.v = reinterpret_cast<const float4 *>(V)[e];
  AlphaPack al;
#pragma unroll
  for (int j = 0; j < kLzWin; ++j) al.a[j] = alpha[j];
  const SlowReplay o = lazy_replay_slow(y, j0, j1, al, two_l2);
  x = o.x;
#pragma unroll
  for (int j = 0; j < kLzWin; ++j)
    if (j >= j0 && j < j1) sq[j] = o.sq[j];
}

__device__ __forceinline__ void lazy_alphas(const LazyArgs &a, int w0, int nj, float (&alpha)[kLzWin]) {
#pragma unroll
  for (int j = 0; j < kLzWin; ++j) alpha[j] = (j < nj && w0 + j < a.n_steps) ? a.sched[w0 + j].alpha : 0.f;
}

// the distinct row a half-wave of the chunk-table grid owns (first chunk of a row's run), or -1.
// kAnimeFirst (the sparse step): the anime table's chunk slots come first in the grid, as in k_bwd — the rows with
// many chunks are anime rows; the catch-up keeps the user chunks first (they are where ITS work is, and the slice of
// them that rides in the head launch is cut from the front of the grid).
// The count word and the chunk record come in ONE round trip: the record index is clamped into the table's slots, and
// a record past the count is dropped unread.
template <bool kAnimeFirst = false>
__device__ __forceinline__ int lazy_chunk_row(const LazyArgs &a, int step, int bid, int &gc, int &nch) {
  const int hw = bid * 8 + (threadIdx.x >> 5);
  const bool flip = kAnimeFirst && a.tables == 2;
  const int T = flip ? (hw < a.capC ? 1 : 0) : (hw >= a.capC ? 1 : 0);
  const int c = hw >= a.capC ? hw - a.capC : hw;
  Slot sl = slot_of(a.arena, a.slot_bytes, a.cap, a.capC, step % a.arena_steps);
  int4 rec = sl.chunks[T * a.capC + min(c, a.capC - 1)];
  int nT = sl.nchunks[T];
  asm volatile("" : "+v"(nT), "+v"(rec.x), "+v"(rec.w));  // both loads are issued here (hipcc sinks rec.x behind the test)
  if (hw >= a.tables * a.capC || c >= nT) return -1;
  if (rec.w <= 0) return -1;
  gc = T * a.capC + c;
  nch = rec.w;
  return rec.x;
}

// the rows batch `step` touches take their pending L2-only steps, so that fwd / bwd of that step read current rows.
// skip_mark > 0: rows whose mark equals it belong to the batch the sparse step of the SAME launch is updating —
// not ours (that half of the launch brings them to `step` itself)
__device__ __forceinline__ void lazy_catchup_row(const LazyArgs &a, int step, int w0, int bid, int skip_mark) {
  const int l = threadIdx.x & 31;
  int gc, nch;
  const int row = lazy_chunk_row(a, step, bid, gc, nch);
  if (row < 0) return;
  // the row's mark, step word and W / M / V are requested TOGETHER: the two words only say whether the row needs
  // anything, and waiting for them before asking for the row costs every stale row one more memory round trip on a
  // path that is nothing but round trips (rows that turn out current — the popular anime rows — cost 1.5 KB each)
  const size_t e = (size_t)row * kRowVec + l;
  const int mk = skip_mark > 0 ? a.z.mark[row] : 0;
  const int ta = a.z.row_step[row];
  Row3 x;
  x.w = reinterpret_cast<const float4 *>(a.W)[e];
  x.m = reinterpret_cast<const float4 *>(a.M)[e];
  x.v = reinterpret_cast<const float4 *>(a.V)[e];
  if (skip_mark > 0 && mk == skip_mark) return;
  if (ta >= step) return;
  float alpha[kLzWin], sq[kLzWin];
  lazy_alphas(a, w0, step - w0, alpha);
#pragma unroll
  for (int j = 0; j < kLzWin; ++j) sq[j] = 0.f;
  lazy_replay<false>(x, ta - w0, step - w0, alpha, a.two_l2, LzBound{}, sq, a.W, a.M, a.V, e);
  reinterpret_cast<float4 *>(a.W)[e] = x.w;
  reinterpret_cast<float4 *>(a.M)[e] = x.m;
  reinterpret_cast<float4 *>(a.V)[e] = x.v;
  float mine = 0.f;
#pragma unroll
  for (int j = 0; j < kLzWin; ++j) {
    const float t = halfwave_sum(sq[j]);
    if (l == j) mine = t;
  }
  if (l >= ta - w0 && l < step - w0) a.z.rowsq[(size_t)row * kLzWin + l] = mine;
  if (l == 0) a.z.row_step[row] = step;
}

}  // namespace anirec
