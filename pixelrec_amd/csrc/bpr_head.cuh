// bpr_head.cuh -- the masked BPR loss head of the sequence models, once: the stand-alone kernels (bpr_loss.hip) and the head fused
// into the block's last LayerNorm (layernorm.hip) form their ids, rows, loss term, coefficient and gradient row here, so
// the two forms use the same formulas in the same order of operations by construction.  No kernel lives here.
//
// Reference sasrec.py:88-92, per position (b, t) with x = pos - neg, s = sigmoid(x) in the naive form 1 / (1 + exp(-x)):
//     lossrow = -log(s + 1e-8) * mask[b, t]
//     coef    = d loss / d x = -(mask / B) * s (1 - s) / (s + 1e-8) * grad_scale [* grad_scale_dev]
//     d out[b, t, :] = coef * (E[pos_id] - E[neg_id])
// (pair_head.cuh's overflow-safe tails are a different rounding: not used here.)
#pragma once
#include "pxr_common.h"

namespace pxr {

struct BprHead {
  const float* table;      // [n_table, D]
  const int64_t* items;    // ids, see the layout below
  const int64_t* mask;     // [B, L]
  float* pos; float* neg;  // [B*L] scores (fwd: written; bwd: read)
  float* lossrow;          // fwd: [B*L] per-position loss term
  float* coef;             // bwd: [B*L] d loss / d(pos - neg)
  int64_t n_table;
  int B, L;
  float grad_scale;
  const float* grad_scale_dev;  // optional device scalar multiplied in (autograd's upstream gradient)
  // id layout: position t of sequence b scores against items[b*id_bstride + pos_off + t] / [... + neg_off + t].  SASRec's shifted
  // [B, 2, L+1] windows: (2(L+1), 1, L+2); BERT4Rec's aligned [B, 3, L] planes: (3L, L, 2L)
  int64_t id_bstride, pos_off, neg_off;
};

// what every entry point knows of the head; the scores, lossrow / coef and the gradient scale are the caller's
static inline BprHead bpr_head_of(const float* table, int64_t n_table, const int64_t* items, const int64_t* mask, int B, int L,
                                  int64_t id_bstride, int64_t pos_off, int64_t neg_off) {
  BprHead h{};
  h.table = table; h.n_table = n_table; h.items = items; h.mask = mask; h.B = B; h.L = L;
  h.id_bstride = id_bstride; h.pos_off = pos_off; h.neg_off = neg_off;
  return h;
}

#ifdef __HIPCC__
// The id pair of position row = b L + t in two steps, and the table row of an id.  (Their shape is what keeps ln_bwd_kernel's
// registers where they were: the division first, the ids read after the coefficient, the row from scalars and not from the head.)
__device__ __forceinline__ void bpr_bt(const BprHead& h, int row, int& b, int& t) {
  b = row / h.L;
  t = row - b * h.L;
}
// the target's and the negative's id under the head's layout
__device__ __forceinline__ void bpr_ids(const BprHead& h, int b, int t, int64_t& ip, int64_t& in) {
  const int64_t* it = h.items + (int64_t)b * h.id_bstride;
  ip = it[h.pos_off + t];
  in = it[h.neg_off + t];
}
// An id outside the table is an error in the reference (nn.Embedding raises on items, sasrec.py:68): the forward flags it (status,
// from the lanes with flag_lane), then clamps; the backward reads the same ids after that launch and passes status = null.
__device__ __forceinline__ const float* bpr_row(const float* table, int64_t n_table, int64_t id, int D, int32_t* status,
                                                bool flag_lane) {
  return table + checked_id(id, n_table, status, flag_lane) * D;
}

// (The two dot products sp = <o, E[pos]>, sn = <o, E[neg]> -- per float4 (x.x + y.y) + (z.z + w.w), then across a lane's chunks in
// column order -- are written out in bpr_fwd_kernel and ln_fwd_kernel: through a shared helper the compiler pairs the products of
// the two sums into FMAs the other way round and a score moves an ulp; tests/test_gpu_seq_head_bits.py holds both sites.)

// the scores of position row and its loss term (one lane)
__device__ __forceinline__ void bpr_store_loss(const BprHead& h, int row, float sp, float sn) {
  h.pos[row] = sp;
  h.neg[row] = sn;
  const float x = sp - sn;
  const float s = 1.0f / (1.0f + expf(-x));
  h.lossrow[row] = -logf(s + 1e-8f) * (float)h.mask[row];
}

// coef from x = pos - neg of the saved scores.  (Scalars in, not the head: with the struct as the argument ln_bwd_kernel<16> spills.)
__device__ __forceinline__ float bpr_coef(float x, float mask, int B, float grad_scale, const float* grad_scale_dev) {
  const float s = 1.0f / (1.0f + expf(-x));
  float cf = -(mask / (float)B) * (s * (1.0f - s)) / (s + 1e-8f) * grad_scale;
  if (grad_scale_dev) cf *= grad_scale_dev[0];
  return cf;
}

// d out[row, c .. c + 3] = cf (E[pos] - E[neg]); cf == 0 (a masked position) reads no table row
__device__ __forceinline__ float4 bpr_dout4(float cf, const float* ep, const float* en, int c) {
  float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
  if (cf != 0.f) {
    const float4 pv = *reinterpret_cast<const float4*>(ep + c);
    const float4 nv = *reinterpret_cast<const float4*>(en + c);
    d.x = cf * (pv.x - nv.x); d.y = cf * (pv.y - nv.y); d.z = cf * (pv.z - nv.z); d.w = cf * (pv.w - nv.w);
  }
  return d;
}
#endif  // __HIPCC__

}  // namespace pxr
