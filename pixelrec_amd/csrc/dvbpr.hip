// dvbpr.hip -- DVBPR's pair head (reference code/REC/model/PixelNet/dvbpr.py:49-62): VBPR's head without the bias term, with the
// visual rows read from the encoder's output E [M, Dh] -- one row per DISTINCT image of the batch -- through positions.  It lives
// beside vbpr.hip and not inside it: VBPR's two kernels are spelled out by hand to keep their bits (see the notes there), and an
// optional-bias argument would recompile them.  What is shared is pair_head.cuh.
//
// Table: one [1 + U + U + I, Dh] buffer in the reference's registration order -- theta_users row u at 1 + u, gamma_users row u at
// 1 + U + u, gamma_items row i at 1 + 2U + i; row 0 is the spare of the sparse-row machinery.
// rows[6B] (pxr_table_rows_i64) = [gamma row of user b | theta row of user b | gamma rows of item_id.view(-1) | positions
// index.view(-1) into E, base 0].  The first 4B entries are the table's occurrences, three segments with disjoint row ranges.
#include "pair_head.cuh"

namespace pxr {

// x_b = <gu_b, gi+ - gi-> + <tu_b, E[p_b] - E[n_b]> as (s+ - s-), loss row = -log sigmoid(x_b) (no 1e-8: dvbpr.py:61).  One wave per b.
__global__ void __launch_bounds__(256) dvbpr_pair_fwd_kernel(const f32x4* __restrict__ table, const int64_t* __restrict__ rows,
                                                              const f32x4* __restrict__ E, int dv, int B, float* __restrict__ coef,
                                                              float* __restrict__ lossrow) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t B64 = B;
  const f32x4* gu = table + rows[b] * dv;
  const f32x4* tu = table + rows[B64 + b] * dv;
  const f32x4* ip = table + rows[2 * B64 + 2 * (int64_t)b] * dv;
  const f32x4* in = table + rows[2 * B64 + 2 * (int64_t)b + 1] * dv;
  const f32x4* ep = E + rows[4 * B64 + 2 * (int64_t)b] * dv;
  const f32x4* en = E + rows[4 * B64 + 2 * (int64_t)b + 1] * dv;
  float sp = 0.f, sn = 0.f;
  for (int c = lane; c < dv; c += 64) {
    const f32x4 u = gu[c], m = tu[c];
    sp += dot4(u, ip[c]) + dot4(m, ep[c]);
    sn += dot4(u, in[c]) + dot4(m, en[c]);
  }
  sp = wave_sum(sp);
  sn = wave_sum(sn);
  if (lane != 0) return;
  float lr, cf;
  bpr_tail_log_outside(sp - sn, B, 0.f, lr, cf);
  lossrow[b] = lr;
  coef[b] = cf;
}

struct DvbprBwdArgs {
  const f32x4* table;
  const int64_t* rows;         // [6B]
  const f32x4* E;              // [M, dv]
  const float* coef;           // [B]
  int dv, B;
  int64_t M;
  float gscale;
  const float* gscale_dev;
  f32x4* dE;                   // [M, dv]
  int64_t* sp_idx;             // [4B]
  f32x4* sp_rows;              // [4B, dv]
  int32_t* sp_n;
};

// One wave per output row, c_b = coef[b] * grad_scale * (*grad_scale_dev):
//   o < 4B: the sparse table gradient of occurrence o (pair_head.cuh's first-occurrence scheme inside the occurrence's own segment):
//     gamma row of user b: c_b (gi+ - gi-);  theta row of user b: c_b (E[p_b] - E[n_b]);  item row (b, t): +-c_b gu_b;
//   o = 4B + m: dE[m, :] = sum over the positions k of index.view(-1) with index[k] == m, ascending k, of +-c_b tu_b -- the dense
//     segment sum of de[2b + t] = +-c_b tu_b into the distinct images' rows; a row no position names gets +0.0.  Position 0 is a
//     real image and is summed like every other.
template <int CH>
__global__ void __launch_bounds__(256) dvbpr_pair_bwd_kernel(DvbprBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int B = a.B, n_occ = 4 * a.B;
  if (o == 0 && lane == 0) a.sp_n[0] = n_occ;
  if (o >= n_occ + a.M) return;
  const float g = grad_scale(a.gscale, a.gscale_dev);
  f32x4 s[CH];
  row_zero(s);
  if (o >= n_occ) {
    const int64_t m = o - n_occ;
    const int64_t* pos = a.rows + 4 * (int64_t)B;
    for_each_occurrence(pos, 0, 2 * B, m, lane, [&](int kk) {
      const int b = kk >> 1;
      const float c = (kk & 1) ? -(a.coef[b] * g) : a.coef[b] * g;
      row_add_scaled(s, c, a.table + a.rows[B + b] * a.dv, a.dv, lane);
    });
    row_store(s, a.dE + m * a.dv, a.dv, lane);
    return;
  }
  const int oi = (int)o;
  const int seg_lo = oi < B ? 0 : oi < 2 * B ? B : 2 * B;
  const int seg_hi = oi < B ? B : oi < 2 * B ? 2 * B : n_occ;
  const int64_t node = a.rows[oi];
  f32x4* dst = a.sp_rows + o * a.dv;
  if (!is_first_occurrence(a.rows, seg_lo, oi, node, lane)) {
    row_store(s, dst, a.dv, lane);
    if (lane == 0) a.sp_idx[oi] = 0;
    return;
  }
  for_each_occurrence(a.rows, oi, seg_hi, node, lane, [&](int kk) {
    if (kk < B) {
      const float c = a.coef[kk] * g;
      row_add_scaled_diff(s, c, a.table + a.rows[2 * B + 2 * (int64_t)kk] * a.dv, a.table + a.rows[2 * B + 2 * (int64_t)kk + 1] * a.dv,
                          a.dv, lane);
    } else if (kk < 2 * B) {
      const int b = kk - B;
      const float c = a.coef[b] * g;
      row_add_scaled_diff(s, c, a.E + a.rows[4 * (int64_t)B + 2 * (int64_t)b] * a.dv, a.E + a.rows[4 * (int64_t)B + 2 * (int64_t)b + 1] * a.dv,
                          a.dv, lane);
    } else {
      const int j = kk - 2 * B, b = j >> 1;
      const float c = (j & 1) ? -(a.coef[b] * g) : a.coef[b] * g;
      row_add_scaled(s, c, a.table + a.rows[b] * a.dv, a.dv, lane);
    }
  });
  row_store(s, dst, a.dv, lane);
  if (lane == 0) a.sp_idx[oi] = node;
}

}  // namespace pxr

using namespace pxr;

extern "C" int pxr_dvbpr_pair_fwd_f32(const float* table, const int64_t* rows, const float* E, int Dh, int B, float* coef,
                                      float* lossrow, float* loss, void* stream) {
  PXR_REQUIRE(table && rows && E && coef && lossrow && loss, "pxr_dvbpr_pair_fwd_f32: null pointer");
  PXR_REQUIRE(Dh > 0 && Dh % 4 == 0 && Dh <= 4096, "pxr_dvbpr_pair_fwd_f32: need Dh %% 4 == 0 and 0 < Dh <= 4096 (Dh=%d)", Dh);
  PXR_REQUIRE(B > 0 && B <= (1 << 26), "pxr_dvbpr_pair_fwd_f32: bad batch size %d", B);
  PXR_REQUIRE((((uintptr_t)table | (uintptr_t)E) & 15) == 0, "pxr_dvbpr_pair_fwd_f32: operands must be 16-byte aligned");
  hipLaunchKernelGGL(dvbpr_pair_fwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)table, rows,
                     (const f32x4*)E, Dh / 4, B, coef, lossrow);
  const int rc = pxr_check_launch("pxr_dvbpr_pair_fwd_f32");
  if (rc) return rc;
  return pxr_bpr_loss_reduce(lossrow, B, 1, loss, stream);        // loss = (1/B) sum_b lossrow[b], fixed order
}

extern "C" int pxr_dvbpr_pair_bwd_f32(const float* table, const int64_t* rows, const float* E, int64_t M, const float* coef, int Dh,
                                      int B, float grad_scale, const float* grad_scale_dev, float* dE, int64_t* sp_idx,
                                      float* sp_rows, int32_t* sp_n, int64_t cap, void* stream) {
  PXR_REQUIRE(table && rows && E && coef && dE && sp_idx && sp_rows && sp_n, "pxr_dvbpr_pair_bwd_f32: null pointer");
  PXR_REQUIRE(Dh > 0 && Dh % 4 == 0 && Dh <= 4096, "pxr_dvbpr_pair_bwd_f32: need Dh %% 4 == 0 and 0 < Dh <= 4096 (Dh=%d)", Dh);
  PXR_REQUIRE(B > 0 && B <= (1 << 26), "pxr_dvbpr_pair_bwd_f32: bad batch size %d", B);
  PXR_REQUIRE(M > 0 && M < (1ll << 31), "pxr_dvbpr_pair_bwd_f32: bad row count of E (M=%lld)", (long long)M);
  PXR_REQUIRE(cap >= 4 * (int64_t)B, "pxr_dvbpr_pair_bwd_f32: sparse capacity %lld < 4B = %lld", (long long)cap, 4 * (long long)B);
  PXR_REQUIRE((((uintptr_t)table | (uintptr_t)E | (uintptr_t)dE | (uintptr_t)sp_rows) & 15) == 0,
              "pxr_dvbpr_pair_bwd_f32: operands must be 16-byte aligned");
  DvbprBwdArgs a{};
  a.table = (const f32x4*)table; a.rows = rows; a.E = (const f32x4*)E; a.coef = coef; a.dv = Dh / 4; a.B = B; a.M = M;
  a.gscale = grad_scale; a.gscale_dev = grad_scale_dev; a.dE = (f32x4*)dE;
  a.sp_idx = sp_idx; a.sp_rows = (f32x4*)sp_rows; a.sp_n = sp_n;
  const int64_t waves = 4 * (int64_t)B + M;
  dispatch_ch<16>(a.dv, [&](auto ch) {
    hipLaunchKernelGGL(dvbpr_pair_bwd_kernel<decltype(ch)::value>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  });
  return pxr_check_launch("pxr_dvbpr_pair_bwd_f32");
}
