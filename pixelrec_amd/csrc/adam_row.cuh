// adam_row.cuh -- the per-element AdamW step and the apply of one gradient row to a lazily updated table row, shared by the
// kernels that update table rows: adamw.hip (dense sweep, lazy replay, lazy apply) and embed_grad.hip (the segment sum that applies
// the row it has just summed).  No kernel lives here.  Every kernel that updates a row goes through these bodies, so all of them
// produce the same bits.
#pragma once
#include "pxr_common.h"

namespace pxr {

struct AdamHyper {
  float decay;        // 1 - lr*wd
  float one_m_b1;     // 1 - beta1
  float b2;           // beta2
  float one_m_b2;     // 1 - beta2
  float step_size;    // lr / (1 - beta1^t)
  float inv_sqrt_bc2; // 1 / sqrt(1 - beta2^t)
  float eps;
};

// the step-independent part of AdamHyper, as the row kernels carry it in their argument blocks
struct AdamConsts { float one_m_b1, b2, one_m_b2, eps; };

#ifdef __HIPCC__
// The operation order is PINNED with explicit fmaf / __fmul_rn so that every kernel that updates a row (dense sweep,
// lazy replay, lazy apply) produces bit-identical results regardless of how the compiler would contract a*b+c.
// sqrt and the division are the hardware's 1-ulp v_sqrt_f32 / v_rcp_f32 (2 quarter-rate instructions) instead of the
// correctly rounded sequences (~25 VALU instructions): a lazily updated row REPLAYS this body once per missed step, so
// its cost is what the lazy schedule pays per step (bench.py `roofline_adamw_rows`).  The update term is <= lr in
// magnitude, so a 1-ulp relative difference in it is ~1e-11 absolute against the +-1e-5 parity bar on parameters.
__device__ __forceinline__ void adam_elem(float& p, float& m, float& v, float g, const AdamHyper& h) {
  p = __fmul_rn(p, h.decay);
  m = fmaf(g - m, h.one_m_b1, m);
  v = fmaf(v, h.b2, __fmul_rn(__fmul_rn(h.one_m_b2, g), g));
  const float denom = fmaf(__builtin_amdgcn_sqrtf(v), h.inv_sqrt_bc2, h.eps);
  p = fmaf(-h.step_size, __fmul_rn(m, __builtin_amdgcn_rcpf(denom)), p);
}
// zero-gradient form of adam_elem (same values bit for bit: fmaf(v, b2, +0) == v * b2, g - m == -m)
__device__ __forceinline__ void adam_elem0(float& p, float& m, float& v, const AdamHyper& h) {
  p = __fmul_rn(p, h.decay);
  m = fmaf(-m, h.one_m_b1, m);
  v = __fmul_rn(v, h.b2);
  const float denom = fmaf(__builtin_amdgcn_sqrtf(v), h.inv_sqrt_bc2, h.eps);
  p = fmaf(-h.step_size, __fmul_rn(m, __builtin_amdgcn_rcpf(denom)), p);
}

// ---- applying a step's gradient row to a table row that is current through the step before (the lazy schedule's apply) ----------
// the scalars of one optimizer step: hs = its entry of the per-step table, {decay, step_size, inv_sqrt_bc2, -}
__device__ __forceinline__ AdamHyper adam_step_hyper(const AdamConsts& c, const float4 hs) {
  AdamHyper h;
  h.one_m_b1 = c.one_m_b1; h.b2 = c.b2; h.one_m_b2 = c.one_m_b2; h.eps = c.eps;
  h.decay = hs.x; h.step_size = hs.y; h.inv_sqrt_bc2 = hs.z;
  return h;
}
// EPL elements of the row, held by one lane
template <int EPL>
__device__ __forceinline__ void adam_apply_row(float (&p)[EPL], float (&m)[EPL], float (&v)[EPL], const float (&g)[EPL],
                                               const AdamHyper& h) {
#pragma unroll
  for (int e = 0; e < EPL; ++e) adam_elem(p[e], m[e], v[e], g[e], h);
}
// the row is now current through step t (ONE lane of the row calls this, after every lane of the row has read last[row])
__device__ __forceinline__ void adam_row_mark(int* __restrict__ last, int64_t row, int t) { last[row] = t; }
#endif  // __HIPCC__

}  // namespace pxr
