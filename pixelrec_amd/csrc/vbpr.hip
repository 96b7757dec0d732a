// vbpr.hip -- VBPR (reference code/REC/model/ViNet/vbpr.py): the gather of frozen feature rows with the visual bias fused, the pair
// head over three tables and the projected features, its backward in sparse row form, the bias projection's gradient, and the
// packing of both sides of the evaluation score into one inner product.  The two projections themselves are the library's GEMMs.
//
// Table: one [1 + U + I + U, Dh] buffer in the reference's parameter order -- user_id_embedding row u at 1 + u,
// item_id_embedding row i at 1 + U + i, user_modal_embedding row u at 1 + U + I + u.  Row 0 is a spare that nothing reads: the
// sparse-row machinery (embed_grad.hip, adamw.hip) treats id 0 as padding / an empty slot, and VBPR has no padding id.
//
// A step's occurrences are laid out as rows[4B] = [id row of user b | modal row of user b | id rows of item.view(-1): (i+_b, i-_b)],
// three segments whose row ranges are disjoint.  The sparse table gradient has one slot per occurrence, summed by pair_head.cuh's
// first-occurrence scheme: (row, sum) in the slot of a row's first occurrence, (0, zeros) in the others.
#include "pair_head.cuh"

namespace pxr {

// out[r, :] = feat[item[r], :] and beta[r] = <feat[item[r], :], wb> from the same registers: the feature row is read once.  One
// wave per row.  item == NULL: row r itself (the whole catalogue); out == NULL: beta only (compute_item_all's total_visual_bias).
__global__ void __launch_bounds__(256) vbpr_gather_kernel(const f32x4* __restrict__ feat, int64_t n_items, int fv,
                                                           const int64_t* __restrict__ item, int64_t n, const f32x4* __restrict__ wb,
                                                           f32x4* __restrict__ out, float* __restrict__ beta, int32_t* status) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const f32x4* src = feat + checked_id(item ? item[r] : r, n_items, status, lane == 0) * fv;
  float s = 0.f;
  for (int c = lane; c < fv; c += 64) {
    const f32x4 v = src[c];
    if (out) out[r * fv + c] = v;
    s += dot4(v, wb[c]);
  }
  s = wave_sum(s);
  if (lane == 0) beta[r] = s;
}

// s_{b,t} = <uid_b, iid_{b,t}> + <um_b, e_{b,t}> + beta_{b,t} with the id rows straight from the table; x_b = s_{b,0} - s_{b,1};
// into the tail with the 1e-8 inside the log (vbpr.py forward).  One wave per b; two terms per side, so the loop is its own.  The
// tail is spelled out here: with it inlined from pair_head.cuh the compiler fuses the loop's multiply-adds in another order and
// x_b moves by an ulp (profiles/pair_head/README.md).
__global__ void __launch_bounds__(256) vbpr_pair_fwd_kernel(const f32x4* __restrict__ table, const int64_t* __restrict__ rows,
                                                             const f32x4* __restrict__ e, const float* __restrict__ beta, int dv, int B,
                                                             float* __restrict__ coef, float* __restrict__ lossrow) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const f32x4* uid = table + rows[b] * dv;
  const f32x4* um = table + rows[B + b] * dv;
  const f32x4* ip = table + rows[2 * (int64_t)B + 2 * (int64_t)b] * dv;
  const f32x4* in = table + rows[2 * (int64_t)B + 2 * (int64_t)b + 1] * dv;
  const f32x4* ep = e + 2 * (int64_t)b * dv;
  const f32x4* en = ep + dv;
  float sp = 0.f, sn = 0.f;
  for (int c = lane; c < dv; c += 64) {
    const f32x4 u = uid[c], m = um[c];
    sp += dot4(u, ip[c]) + dot4(m, ep[c]);
    sn += dot4(u, in[c]) + dot4(m, en[c]);
  }
  sp = wave_sum(sp);
  sn = wave_sum(sn);
  if (lane != 0) return;
  const float x = (sp + beta[2 * (int64_t)b]) - (sn + beta[2 * (int64_t)b + 1]);
  const float ex = expf(-fabsf(x));                                         // bpr_tail_log_inside, kept in place (see above)
  const float sig = x >= 0.f ? 1.f / (1.f + ex) : ex / (1.f + ex);
  const float sneg = x >= 0.f ? ex / (1.f + ex) : 1.f / (1.f + ex);
  lossrow[b] = -logf(1e-8f + sig);
  coef[b] = -(sig * sneg / (1e-8f + sig)) / (float)B;
}

// The head's backward from coef, one wave per occurrence o of rows[4B], c_b = coef[b] * grad_scale * (*grad_scale_dev):
//   every item occurrence j = o - 2B (sample b = j / 2, sign + for the positive, - for the negative) first writes the operand of
//   the weight-gradient GEMM de[j, :] = +-c_b um_b and csign[j] = +-c_b (the bias projection's column sum reads it);
//   then the sparse table gradient, contribution of occurrence k:
//     id row of user b: c_b (iid+_b - iid-_b);  modal row of user b: c_b (e+_b - e-_b);  item row (b, t): +-c_b uid_b.
// Rows of different segments never coincide, so both scans stay inside the occurrence's own segment.
// The first-occurrence scheme of pair_head.cuh is spelled out here: through the shared walk and register row the compiler fuses
// the multiply-adds of vbpr_pair_bwd_kernel<2> in another order and the row sums move by an ulp (profiles/pair_head/README.md).
struct VbprBwdArgs {
  const f32x4* table;
  const int64_t* rows;
  const f32x4* e;              // [2B, dv]
  const float* coef;           // [B]
  int dv, B;
  float gscale;
  const float* gscale_dev;
  f32x4* de;                   // [2B, dv]
  float* csign;                // [2B]
  int64_t* sp_idx;             // [4B]
  f32x4* sp_rows;              // [4B, dv]
  int32_t* sp_n;
};

template <int CH>
__global__ void __launch_bounds__(256) vbpr_pair_bwd_kernel(VbprBwdArgs a) {
  const int lane = threadIdx.x & 63;
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int B = a.B, n_occ = 4 * a.B;
  if (o == 0 && lane == 0) a.sp_n[0] = n_occ;
  if (o >= n_occ) return;
  const float g = grad_scale(a.gscale, a.gscale_dev);
  if (o >= 2 * B) {
    const int j = o - 2 * B, b = j >> 1;
    const float cs = (j & 1) ? -(a.coef[b] * g) : a.coef[b] * g;
    const f32x4* um = a.table + a.rows[B + b] * a.dv;
    f32x4* d = a.de + (int64_t)j * a.dv;
#pragma unroll
    for (int h = 0; h < CH; ++h) {
      const int ch = lane + h * 64;
      if (ch < a.dv) d[ch] = cs * um[ch];
    }
    if (lane == 0) a.csign[j] = cs;
  }
  const int seg_lo = o < B ? 0 : o < 2 * B ? B : 2 * B;
  const int seg_hi = o < B ? B : o < 2 * B ? 2 * B : n_occ;
  const int64_t node = a.rows[o];
  bool first = true;
  for (int k0 = seg_lo; k0 < o && first; k0 += 64) {
    const int k = k0 + lane;
    if (__ballot(k < o && a.rows[k] == node)) first = false;
  }
  f32x4* dst = a.sp_rows + (int64_t)o * a.dv;
  if (!first) {
#pragma unroll
    for (int h = 0; h < CH; ++h) {
      const int ch = lane + h * 64;
      if (ch < a.dv) dst[ch] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (lane == 0) a.sp_idx[o] = 0;
    return;
  }
  f32x4 s[CH];
#pragma unroll
  for (int h = 0; h < CH; ++h) s[h] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = o; k0 < seg_hi; k0 += 64) {
    const int k = k0 + lane;
    unsigned long long m = __ballot(k < seg_hi && a.rows[k] == node);
    while (m) {
      const int kk = k0 + __builtin_ctzll(m);
      m &= m - 1;
      const f32x4 *p, *n;                      // contribution = c (p - n), n == NULL: c p
      float c;
      if (kk < 2 * B) {
        const int b = kk < B ? kk : kk - B;
        c = a.coef[b] * g;
        if (kk < B) {
          p = a.table + a.rows[2 * B + 2 * (int64_t)b] * a.dv;
          n = a.table + a.rows[2 * B + 2 * (int64_t)b + 1] * a.dv;
        } else {
          p = a.e + 2 * (int64_t)b * a.dv;
          n = p + a.dv;
        }
      } else {
        const int j = kk - 2 * B, b = j >> 1;
        c = (j & 1) ? -(a.coef[b] * g) : a.coef[b] * g;
        p = a.table + a.rows[b] * a.dv;
        n = nullptr;
      }
      if (n) {
#pragma unroll
        for (int h = 0; h < CH; ++h) {
          const int ch = lane + h * 64;
          if (ch < a.dv) s[h] += c * (p[ch] - n[ch]);
        }
      } else {
#pragma unroll
        for (int h = 0; h < CH; ++h) {
          const int ch = lane + h * 64;
          if (ch < a.dv) s[h] += c * p[ch];
        }
      }
    }
  }
#pragma unroll
  for (int h = 0; h < CH; ++h) {
    const int ch = lane + h * 64;
    if (ch < a.dv) dst[ch] = s[h];
  }
  if (lane == 0) a.sp_idx[o] = node;
}

// d w_b [F] = sum_r csign[r] x[r, :] over the gathered rows x [R, F].  A workgroup owns VB_CC float4 columns and walks every row
// with VB_RL row lanes; the VB_RL partial sums of a column are added in lane order through LDS (one fixed summation order).
constexpr int VB_CC = 8, VB_RL = 32;

__global__ void __launch_bounds__(256) vbpr_bias_grad_kernel(const f32x4* __restrict__ x, const float* __restrict__ csign, int R, int fv,
                                                              f32x4* __restrict__ dwb) {
  __shared__ f32x4 red[VB_RL][VB_CC];
  const int cc = threadIdx.x % VB_CC, rl = threadIdx.x / VB_CC;
  const int c4 = blockIdx.x * VB_CC + cc;
  const bool ok = c4 < fv;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (ok)
    for (int r = rl; r < R; r += VB_RL) s += csign[r] * x[(int64_t)r * fv + c4];
  red[rl][cc] = s;
  __syncthreads();
  if (rl != 0 || !ok) return;
  f32x4 t = red[0][cc];
#pragma unroll
  for (int k = 1; k < VB_RL; ++k) t += red[k][cc];
  dwb[c4] = t;
}

// out[r, :] = [a[ra, :] | b[rb, :] | s_r | 0 ...] of width 4 pv (ra = a_rows ? a_rows[r] : r, rb likewise; s_r = s ? s[r] : 1): the
// item side (item id row | projected feature | visual bias) and the query side (user id row | user modal row | 1) of the score
// as one inner product.  One wave per row.
__global__ void __launch_bounds__(256) vbpr_pack_kernel(const f32x4* __restrict__ a, const int64_t* __restrict__ a_rows,
                                                         const f32x4* __restrict__ b, const int64_t* __restrict__ b_rows,
                                                         const float* __restrict__ s, int64_t R, int dv, int pv, f32x4* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const f32x4* pa = a + (a_rows ? a_rows[r] : r) * dv;
  const f32x4* pb = b + (b_rows ? b_rows[r] : r) * dv;
  f32x4* dst = out + r * pv;
  for (int c = lane; c < dv; c += 64) {
    dst[c] = pa[c];
    dst[dv + c] = pb[c];
  }
  for (int c = 2 * dv + lane; c < pv; c += 64) dst[c] = f32x4{c == 2 * dv ? (s ? s[r] : 1.f) : 0.f, 0.f, 0.f, 0.f};
}

}  // namespace pxr

using namespace pxr;

extern "C" int pxr_vbpr_gather_f32(const float* feat, int64_t n_items, int F, const int64_t* item, int64_t n, const float* wb,
                                   float* out, float* beta, void* stream) {
  PXR_REQUIRE(feat && wb && beta, "pxr_vbpr_gather_f32: null pointer");
  PXR_REQUIRE(F > 0 && F % 4 == 0, "pxr_vbpr_gather_f32: need F %% 4 == 0 (F=%d)", F);
  PXR_REQUIRE(n_items > 0 && n > 0 && n < (1ll << 31) && (item || n <= n_items), "pxr_vbpr_gather_f32: bad row count");
  PXR_REQUIRE((((uintptr_t)feat | (uintptr_t)wb | (uintptr_t)out) & 15) == 0, "pxr_vbpr_gather_f32: operands must be 16-byte aligned");
  hipLaunchKernelGGL(vbpr_gather_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)feat, n_items,
                     F / 4, item, n, (const f32x4*)wb, (f32x4*)out, beta, pxr_status_word());
  return pxr_check_launch("pxr_vbpr_gather_f32");
}

extern "C" int pxr_vbpr_pair_fwd_f32(const float* table, const int64_t* rows, const float* e, const float* beta, int Dh, int B,
                                     float* coef, float* lossrow, float* loss, void* stream) {
  PXR_REQUIRE(table && rows && e && beta && coef && lossrow && loss, "pxr_vbpr_pair_fwd_f32: null pointer");
  PXR_REQUIRE(Dh > 0 && Dh % 4 == 0 && Dh <= 4096, "pxr_vbpr_pair_fwd_f32: need Dh %% 4 == 0 and 0 < Dh <= 4096 (Dh=%d)", Dh);
  PXR_REQUIRE(B > 0 && B <= (1 << 26), "pxr_vbpr_pair_fwd_f32: bad batch size %d", B);
  PXR_REQUIRE((((uintptr_t)table | (uintptr_t)e) & 15) == 0, "pxr_vbpr_pair_fwd_f32: operands must be 16-byte aligned");
  hipLaunchKernelGGL(vbpr_pair_fwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)table, rows,
                     (const f32x4*)e, beta, Dh / 4, B, coef, lossrow);
  const int rc = pxr_check_launch("pxr_vbpr_pair_fwd_f32");
  if (rc) return rc;
  return pxr_bpr_loss_reduce(lossrow, B, 1, loss, stream);        // loss = (1/B) sum_b lossrow[b], fixed order
}

extern "C" int pxr_vbpr_pair_bwd_f32(const float* table, const int64_t* rows, const float* e, const float* coef, int Dh, int B,
                                     float grad_scale, const float* grad_scale_dev, float* de, float* csign, int64_t* sp_idx,
                                     float* sp_rows, int32_t* sp_n, int64_t cap, void* stream) {
  PXR_REQUIRE(table && rows && e && coef && de && csign && sp_idx && sp_rows && sp_n, "pxr_vbpr_pair_bwd_f32: null pointer");
  PXR_REQUIRE(Dh > 0 && Dh % 4 == 0 && Dh <= 4096, "pxr_vbpr_pair_bwd_f32: need Dh %% 4 == 0 and 0 < Dh <= 4096 (Dh=%d)", Dh);
  PXR_REQUIRE(B > 0 && B <= (1 << 26), "pxr_vbpr_pair_bwd_f32: bad batch size %d", B);
  PXR_REQUIRE(cap >= 4 * (int64_t)B, "pxr_vbpr_pair_bwd_f32: sparse capacity %lld < 4B = %lld", (long long)cap, 4 * (long long)B);
  PXR_REQUIRE((((uintptr_t)table | (uintptr_t)e | (uintptr_t)de | (uintptr_t)sp_rows) & 15) == 0,
              "pxr_vbpr_pair_bwd_f32: operands must be 16-byte aligned");
  VbprBwdArgs a{};
  a.table = (const f32x4*)table; a.rows = rows; a.e = (const f32x4*)e; a.coef = coef; a.dv = Dh / 4; a.B = B;
  a.gscale = grad_scale; a.gscale_dev = grad_scale_dev; a.de = (f32x4*)de; a.csign = csign;
  a.sp_idx = sp_idx; a.sp_rows = (f32x4*)sp_rows; a.sp_n = sp_n;
  dispatch_ch<16>(a.dv, [&](auto ch) {                             // 4B occurrences, 4 waves per workgroup
    hipLaunchKernelGGL(vbpr_pair_bwd_kernel<decltype(ch)::value>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
  });
  return pxr_check_launch("pxr_vbpr_pair_bwd_f32");
}

extern "C" int pxr_vbpr_bias_grad_f32(const float* x, const float* csign, int R, int F, float* dwb, void* stream) {
  PXR_REQUIRE(x && csign && dwb, "pxr_vbpr_bias_grad_f32: null pointer");
  PXR_REQUIRE(R > 0 && F > 0 && F % 4 == 0, "pxr_vbpr_bias_grad_f32: need R > 0 and F %% 4 == 0 (R=%d, F=%d)", R, F);
  PXR_REQUIRE((((uintptr_t)x | (uintptr_t)dwb) & 15) == 0, "pxr_vbpr_bias_grad_f32: operands must be 16-byte aligned");
  const int fv = F / 4;
  hipLaunchKernelGGL(vbpr_bias_grad_kernel, dim3((unsigned)((fv + VB_CC - 1) / VB_CC)), dim3(256), 0, (hipStream_t)stream,
                     (const f32x4*)x, csign, R, fv, (f32x4*)dwb);
  return pxr_check_launch("pxr_vbpr_bias_grad_f32");
}

extern "C" int pxr_vbpr_pack_f32(const float* a, const int64_t* a_rows, const float* b, const int64_t* b_rows, const float* s,
                                 int64_t R, int Dh, int Dp, float* out, void* stream) {
  PXR_REQUIRE(a && b && out, "pxr_vbpr_pack_f32: null pointer");
  PXR_REQUIRE(Dh > 0 && Dh % 4 == 0 && Dh <= 4096, "pxr_vbpr_pack_f32: need Dh %% 4 == 0 and 0 < Dh <= 4096 (Dh=%d)", Dh);
  PXR_REQUIRE(Dp % 4 == 0 && Dp > 2 * Dh, "pxr_vbpr_pack_f32: need Dp %% 4 == 0 and Dp > 2 Dh (Dp=%d, Dh=%d)", Dp, Dh);
  PXR_REQUIRE(R > 0 && R < (1ll << 31), "pxr_vbpr_pack_f32: bad row count");
  PXR_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) == 0, "pxr_vbpr_pack_f32: operands must be 16-byte aligned");
  hipLaunchKernelGGL(vbpr_pack_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)a, a_rows,
                     (const f32x4*)b, b_rows, s, R, Dh / 4, Dp / 4, (f32x4*)out);
  return pxr_check_launch("pxr_vbpr_pack_f32");
}
