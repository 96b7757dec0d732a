// bpr_loss.hip -- the SASRec training head (K13): pairwise loss against ONE sampled negative per position.
//
// Reference sasrec.py:88-92:
//     pos = (out * E[items[:,0,1:]]).sum(-1);  neg = (out * E[items[:,1,1:]]).sum(-1)
//     loss = mean_b( - sum_t log(sigmoid(pos - neg) + 1e-8) * masked_index[b,t] )
// Fused with the target-row gathers: the [B,2,L+1,D] gathered tensor of sasrec.py:68 is never materialised,
// each target row is read straight from the table by the wave that needs it (2 KB coalesced per row at D=512).
// One 64-lane wave per (b,t) position; the scalar loss is produced by a fixed-order second stage (deterministic)
// and STAYS ON THE DEVICE (the reference syncs the host every step with .item(), trainer.py:121).
//
// Backward: x = pos - neg, s = sigmoid(x);  dL/dx = -(mask/B) * s(1-s)/(s+1e-8) * grad_scale =: coef[b,t]
//     d out[b,t,:]   = coef * (E[pos_id] - E[neg_id])
//     d E[pos_id,:] += coef * out[b,t,:],  d E[neg_id,:] -= coef * out[b,t,:]   (done by embed_grad.hip from coef)
#include "bpr_head.cuh"
#include "reduce_multi.cuh"

namespace pxr {

// the head (bpr_head.cuh) on out [B*L, D], one wave per position
__global__ void __launch_bounds__(256) bpr_fwd_kernel(BprHead h, const float* out, int D, int32_t* status) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  if (r >= h.B * h.L) return;
  int b, t;
  int64_t ip, in;
  bpr_bt(h, r, b, t);
  bpr_ids(h, b, t, ip, in);
  const float* ep = bpr_row(h.table, h.n_table, ip, D, status, lane == 0);
  const float* en = bpr_row(h.table, h.n_table, in, D, status, lane == 0);
  const float* o = out + (int64_t)r * D;
  float sp = 0.f, sn = 0.f;
  // (written out here and in ln_fwd_kernel, not shared: bpr_head.cuh says why)
  for (int c = lane * 4; c < D; c += 256) {
    const float4 ov = *reinterpret_cast<const float4*>(o + c);
    const float4 pv = *reinterpret_cast<const float4*>(ep + c);
    const float4 nv = *reinterpret_cast<const float4*>(en + c);
    sp += (ov.x * pv.x + ov.y * pv.y) + (ov.z * pv.z + ov.w * pv.w);
    sn += (ov.x * nv.x + ov.y * nv.y) + (ov.z * nv.z + ov.w * nv.w);
  }
  sp = wave_sum(sp);
  sn = wave_sum(sn);
  if (lane == 0) bpr_store_loss(h, r, sp, sn);
}

// loss = (1/B) * sum_b ( sum_t lossrow[b,t] )   single block, fixed order
__global__ void __launch_bounds__(256) bpr_reduce_kernel(const float* __restrict__ lossrow, int B, int L,
                                                         float* __restrict__ loss) {
  __shared__ float red[256];
  pxr_bpr_reduce_block(lossrow, B, L, loss, red, (int)threadIdx.x);   // reduce_multi.cuh: shared with the rider blocks (embed_grad.hip)
}

__global__ void __launch_bounds__(256) bpr_bwd_kernel(BprHead h, float* dout, int D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + wave;
  if (r >= h.B * h.L) return;
  int b, t;
  int64_t ip, in;
  bpr_bt(h, r, b, t);
  const float cf = bpr_coef(h.pos[r] - h.neg[r], (float)h.mask[r], h.B, h.grad_scale, h.grad_scale_dev);
  if (lane == 0) h.coef[r] = cf;
  bpr_ids(h, b, t, ip, in);
  const float* ep = bpr_row(h.table, h.n_table, ip, D, nullptr, false);
  const float* en = bpr_row(h.table, h.n_table, in, D, nullptr, false);
  float* d = dout + (int64_t)r * D;
  for (int c = lane * 4; c < D; c += 256) *reinterpret_cast<float4*>(d + c) = bpr_dout4(cf, ep, en, c);
}

}  // namespace pxr

using namespace pxr;

// loss (device scalar), pos_score / neg_score [B*L].  lossrow is [B*L] scratch.  The id layout (BprHead::id_bstride): SASRec's
// shifted windows pass (2(L+1), 1, L+2); BERT4Rec's aligned masked head, reference IDNet/bert4rec.py:98-111, passes (3L, L, 2L)
// (items [B, 3, L] = masked sequence | original sequence | negatives; masked_index [B, L]).
extern "C" int pxr_bpr_loss_fwd_f32(const float* out, const float* table, int64_t n_table, const int64_t* items,
                                    const int64_t* masked_index, int B, int L, int D, float* pos_score, float* neg_score,
                                    float* lossrow, float* loss, int64_t id_bstride, int64_t pos_off, int64_t neg_off,
                                    void* stream) {
  PXR_REQUIRE(pxr_bpr_layout_ok(L, id_bstride, pos_off, neg_off), "pxr_bpr_loss_fwd_f32: bad id layout");
  PXR_REQUIRE(out && table && items && masked_index && pos_score && neg_score && lossrow && loss,
              "pxr_bpr_loss_fwd_f32: null pointer");
  PXR_REQUIRE(B > 0 && L > 0 && D > 0 && D % 4 == 0, "pxr_bpr_loss_fwd_f32: bad shape");
  BprHead h = bpr_head_of(table, n_table, items, masked_index, B, L, id_bstride, pos_off, neg_off);
  h.pos = pos_score; h.neg = neg_score; h.lossrow = lossrow;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(bpr_fwd_kernel, dim3((B * L + 3) / 4), dim3(256), 0, st, h, out, D, pxr_status_word());
  hipLaunchKernelGGL(bpr_reduce_kernel, dim3(1), dim3(256), 0, st, (const float*)lossrow, B, L, loss);
  return pxr_check_launch("pxr_bpr_loss_fwd_f32");
}

// The second stage alone (pxr_common.h).
int pxr_bpr_loss_reduce(const float* lossrow, int B, int L, float* loss, void* stream) {
  PXR_REQUIRE(lossrow && loss && B > 0 && L > 0, "pxr_bpr_loss_reduce: bad args");
  hipLaunchKernelGGL(bpr_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, lossrow, B, L, loss);
  return pxr_check_launch("pxr_bpr_loss_reduce");
}

// dout [B*L, D] and coef [B*L] from the saved scores; upstream d(loss) = grad_scale * (*grad_scale_dev if given).  The id layout
// is pxr_bpr_loss_fwd_f32's (BERT4Rec: reference IDNet/bert4rec.py:98-113 under autograd).
extern "C" int pxr_bpr_loss_bwd_f32(const float* pos_score, const float* neg_score, const float* table, int64_t n_table,
                                    const int64_t* items, const int64_t* masked_index, int B, int L, int D, float grad_scale,
                                    const float* grad_scale_dev, float* dout, float* coef, int64_t id_bstride,
                                    int64_t pos_off, int64_t neg_off, void* stream) {
  PXR_REQUIRE(pxr_bpr_layout_ok(L, id_bstride, pos_off, neg_off), "pxr_bpr_loss_bwd_f32: bad id layout");
  PXR_REQUIRE(pos_score && neg_score && table && items && masked_index && dout && coef,
              "pxr_bpr_loss_bwd_f32: null pointer");
  PXR_REQUIRE(B > 0 && L > 0 && D > 0 && D % 4 == 0, "pxr_bpr_loss_bwd_f32: bad shape");
  BprHead h = bpr_head_of(table, n_table, items, masked_index, B, L, id_bstride, pos_off, neg_off);
  h.pos = const_cast<float*>(pos_score); h.neg = const_cast<float*>(neg_score); h.coef = coef;
  h.grad_scale = grad_scale; h.grad_scale_dev = grad_scale_dev;
  hipLaunchKernelGGL(bpr_bwd_kernel, dim3((B * L + 3) / 4), dim3(256), 0, (hipStream_t)stream, h, dout, D);
  return pxr_check_launch("pxr_bpr_loss_bwd_f32");
}
