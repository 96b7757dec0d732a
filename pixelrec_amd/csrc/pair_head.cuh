// pair_head.cuh -- the core shared by the pair-wise BPR kernels over float4 rows (mf.hip, vbpr.hip, lightgcn.hip, srgnn.hip,
// curator.hip, acf.hip): the two loss tails, the pair of wave dot products, the deterministic
// first-occurrence segment sum with its register row, the gradient scale and the host's choice of the CH instantiation.  No kernel
// lives here.  A kernel of those files resolves its rows, calls the core and writes its outputs.
//
// The first-occurrence scheme (no sort, no float atomics, bit-identical from run to run): a step's gradient rows are listed per
// OCCURRENCE of a table row, one wave per occurrence o.  The wave scans the ids before o (is_first_occurrence); only the first
// occurrence of a row goes on, visits every occurrence of that row from o to the end of the list in ascending order
// (for_each_occurrence), adds their contributions into a register row (row_zero / row_add_scaled / row_add_scaled_diff) and stores
// the sum (row_store).  What a later occurrence does -- write an empty slot, or nothing -- is the caller's.  The 3B or 4B ids stay in
// L1 / L2.  A register row is CH float4s per lane, chunk lane + 64 h of the row's dv = D / 4; everything here is force-inlined and
// fully unrolled so that it stays in registers.
#pragma once
#include <type_traits>

#include "pxr_common.h"

namespace pxr {

// f(std::integral_constant<int, CH>) for the smallest CH in {1, 2, 4, 8, 16} up to MAXCH whose 64 CH chunks hold a row of dv float4s
// (a wider row takes MAXCH: the entry points bound D)
template <int MAXCH, class F>
static inline void dispatch_ch(int dv, F&& f) {
  static_assert(MAXCH == 8 || MAXCH == 16, "instantiated widths end at 8 or 16 chunks per lane");
  const int ch = (dv + 63) / 64;
  if (ch <= 1) f(std::integral_constant<int, 1>{});
  else if (ch <= 2) f(std::integral_constant<int, 2>{});
  else if (ch <= 4) f(std::integral_constant<int, 4>{});
  else if (ch <= 8 || MAXCH == 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, MAXCH>{});
}

#ifdef __HIPCC__
__device__ __forceinline__ float dot4(const f32x4& p, const f32x4& q) { return p.x * q.x + p.y * q.y + p.z * q.z + p.w * q.w; }

// The two loss tails: x_b -> (lossrow[b], coef[b] = d loss / d x_b) of loss = mean_b lossrow[b].  Both take e = exp(-|x|) <= 1 and
// pick sigmoid(x) and 1 - sigmoid(x) = sigmoid(-x) by the sign of x, so nothing overflows and no 1 - (nearly 1) cancels: every
// value is finite for any |x|.
//   log outside: lossrow = -(1e-8 + log sigmoid(x)), coef = -(1 - sigmoid(x)) / B -- mf.py, lightgcn.py:70-78 and srgnn.py:60-66 add
//     the 1e-8 OUTSIDE the log, where it shifts the loss and leaves the gradient alone; log sigmoid(x) = min(x, 0) - log1p(e).
//     The shift is the argument eps of the five-argument form (momf.py:59 has none: eps = 0).
//   log inside: lossrow = -log(1e-8 + sigmoid(x)), coef = -sigmoid(x)(1 - sigmoid(x)) / (1e-8 + sigmoid(x)) / B -- vbpr.py and
//     curatornet.py:86-88 add it INSIDE, so a badly ranked pair saturates at -log(1e-8) and its gradient fades.
__device__ __forceinline__ void bpr_tail_log_outside(float x, int B, float eps, float& lossrow, float& coef) {
  const float e = expf(-fabsf(x));
  const float ls = fminf(x, 0.f) - log1pf(e);
  const float sneg = x >= 0.f ? e / (1.f + e) : 1.f / (1.f + e);
  lossrow = -(eps + ls);
  coef = -sneg / (float)B;
}
__device__ __forceinline__ void bpr_tail_log_outside(float x, int B, float& lossrow, float& coef) {
  bpr_tail_log_outside(x, B, 1e-8f, lossrow, coef);
}
__device__ __forceinline__ void bpr_tail_log_inside(float x, int B, float& lossrow, float& coef) {
  const float e = expf(-fabsf(x));
  const float sig = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
  const float sneg = x >= 0.f ? e / (1.f + e) : 1.f / (1.f + e);
  lossrow = -logf(1e-8f + sig);
  coef = -(sig * sneg / (1e-8f + sig)) / (float)B;
}

// sp = <u, p>, sn = <u, n> over rows of dv float4s, one wave per sample: lane-strided partial sums, then the wave's totals on every
// lane (all 64 lanes must call)
__device__ __forceinline__ void pair_dots(const f32x4* u, const f32x4* p, const f32x4* n, int dv, int lane, float& sp, float& sn) {
  sp = sn = 0.f;
  for (int c = lane; c < dv; c += 64) {
    const f32x4 uv = u[c];
    sp += dot4(uv, p[c]);
    sn += dot4(uv, n[c]);
  }
  sp = wave_sum(sp);
  sn = wave_sum(sn);
}

// gradient scale of a step: the host's factor times the device's (the loss scale of a graphed step), when there is one
__device__ __forceinline__ float grad_scale(float gscale, const float* gscale_dev) {
  return gscale * (gscale_dev ? gscale_dev[0] : 1.f);
}

// no id of ids[lo, o) equals node (wave-uniform; all 64 lanes must call)
template <class T>
__device__ __forceinline__ bool is_first_occurrence(const T* ids, int lo, int o, T node, int lane) {
  for (int k0 = lo; k0 < o; k0 += 64) {
    const int k = k0 + lane;
    if (__ballot(k < o && ids[k] == node)) return false;
  }
  return true;
}

// f(kk) for every kk in [o, hi) with ids[kk] == node, in ascending kk, on all 64 lanes alike
template <class T, class F>
__device__ __forceinline__ void for_each_occurrence(const T* ids, int o, int hi, T node, int lane, F&& f) {
  for (int k0 = o; k0 < hi; k0 += 64) {
    const int k = k0 + lane;
    unsigned long long m = __ballot(k < hi && ids[k] == node);
    while (m) {
      const int kk = k0 + __builtin_ctzll(m);
      m &= m - 1;
      f(kk);
    }
  }
}

// the register row s: s = 0; s += c p; s += c (p - n); dst = s
template <int CH>
__device__ __forceinline__ void row_zero(f32x4 (&s)[CH]) {
#pragma unroll
  for (int h = 0; h < CH; ++h) s[h] = f32x4{0.f, 0.f, 0.f, 0.f};
}
template <int CH>
__device__ __forceinline__ void row_add_scaled(f32x4 (&s)[CH], float c, const f32x4* p, int dv, int lane) {
#pragma unroll
  for (int h = 0; h < CH; ++h) {
    const int ch = lane + h * 64;
    if (ch < dv) s[h] += c * p[ch];
  }
}
template <int CH>
__device__ __forceinline__ void row_add_scaled_diff(f32x4 (&s)[CH], float c, const f32x4* p, const f32x4* n, int dv, int lane) {
#pragma unroll
  for (int h = 0; h < CH; ++h) {
    const int ch = lane + h * 64;
    if (ch < dv) s[h] += c * (p[ch] - n[ch]);
  }
}
template <int CH>
__device__ __forceinline__ void row_store(const f32x4 (&s)[CH], f32x4* dst, int dv, int lane) {
#pragma unroll
  for (int h = 0; h < CH; ++h) {
    const int ch = lane + h * 64;
    if (ch < dv) dst[ch] = s[h];
  }
}
#endif  // __HIPCC__

}  // namespace pxr
