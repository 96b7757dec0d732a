// pool.hip -- the pooled-history pair models DSSM and FM (reference code/REC/model/IDNet/dssm.py, fm.py): a masked pooling of up to L
// gathered table rows, alone or fused with the pair head, and the head's backward as a COMPACT gradient block.
//
// A sample b has a profile of L row indices (padding = the index `pad_row`), a positive row and a negative row:
//     U_b = sum_l [rows[b, l] != pad_row] table[rows[b, l]]        (l ascending: one fixed order)
//     mean: U_b / (cnt_b + 1e-8f), cnt_b the number of real positions -- an fp32 division, as torch.div does it (dssm.py avg_emb);
//           an empty profile gives exactly 0
//     x_b = <U_b, table[p_b]> - <U_b, table[n_b]>,   loss = -mean_b log(1e-8 + sigmoid(x_b))                  (pair_head.cuh)
// FM's factorisation machine over [profile | p] minus the one over [profile | n] is exactly this x with sum pooling: the
// history-history terms are the same in both scores (fm.py forward, layers.py BaseFactorizationMachine).
//
// Backward: G [3B, D] holds ONE gradient row per sample for all of its L history occurrences (c_b (e[p_b] - e[n_b])) and one per
// target (+- c_b U_b); the pooling weight w_b is applied by the segment sum of embed_grad.hip (MODE_POOL), which points the L
// history occurrences of a sample at that one row.  No [B (L + 2), D] buffer exists.
//
// One wave per sample; a row is CH float4s per lane (chunk lane + 64 h), kept in registers.  No atomics on floats.
#include "pair_head.cuh"

namespace pxr {

struct PoolArgs {
  const f32x4* table;          // [n_table, dv]
  int64_t n_table;
  const int64_t* rows;         // [B, L] profile rows, then (pair kernels) [B, 2] target rows
  int64_t pad_row;             // the profile index that means "no item"
  int B, L, dv, mean;
  f32x4* U;                    // [B, dv]
  float* w;                    // [B] the factor the backward multiplies a history occurrence by
  float* coef;                 // [B] d loss / d x_b                                                      (pair kernels)
  float* lossrow;              // [B]
  float gscale;
  const float* gscale_dev;
  f32x4* G;                    // [3B, dv]
};

// s = the pooled row of sample b (summed, then divided when a.mean); returns w_b.  All 64 lanes call.
template <int CH>
__device__ __forceinline__ float pool_row(const PoolArgs& a, int b, int lane, f32x4 (&s)[CH], int32_t* status) {
  row_zero(s);
  int cnt = 0;
  const int64_t* prof = a.rows + (int64_t)b * a.L;
  for (int l = 0; l < a.L; ++l) {
    const int64_t id = prof[l];                         // wave-uniform
    if (id == a.pad_row) continue;
    const int64_t r = checked_id(id, a.n_table, status, lane == 0);
    row_add_scaled(s, 1.f, a.table + r * a.dv, a.dv, lane);      // 1 x is x: the plain sum
    ++cnt;
  }
  if (!a.mean) return cnt ? 1.f : 0.f;
  const float den = (float)cnt + 1e-8f;                 // == cnt for cnt >= 1; 1e-8 for an empty profile, whose sum is exactly 0
#pragma unroll
  for (int h = 0; h < CH; ++h) s[h] = s[h] / den;
  return cnt ? 1.f / den : 0.f;
}

template <int CH>
__global__ void __launch_bounds__(256) pool_rows_kernel(PoolArgs a, int32_t* status) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  f32x4 s[CH];
  const float w = pool_row(a, b, lane, s, status);
  row_store(s, a.U + (int64_t)b * a.dv, a.dv, lane);
  if (lane == 0) a.w[b] = w;
}

// the pooling, the two dot products against the target rows and the loss tail in one launch
template <int CH>
__global__ void __launch_bounds__(256) pool_pair_fwd_kernel(PoolArgs a, int32_t* status) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  f32x4 s[CH];
  const float w = pool_row(a, b, lane, s, status);
  row_store(s, a.U + (int64_t)b * a.dv, a.dv, lane);
  const int64_t* tgt = a.rows + (int64_t)a.B * a.L + 2 * (int64_t)b;
  const f32x4* p = a.table + checked_id(tgt[0], a.n_table, status, lane == 0) * a.dv;
  const f32x4* n = a.table + checked_id(tgt[1], a.n_table, status, lane == 0) * a.dv;
  float sp = 0.f, sn = 0.f;
#pragma unroll
  for (int h = 0; h < CH; ++h) {
    const int ch = lane + h * 64;
    if (ch < a.dv) {
      sp += dot4(s[h], p[ch]);
      sn += dot4(s[h], n[ch]);
    }
  }
  sp = wave_sum(sp);
  sn = wave_sum(sn);
  if (lane == 0) {
    a.w[b] = w;
    bpr_tail_log_inside(sp - sn, a.B, a.lossrow[b], a.coef[b]);
  }
}

// G[b] = c_b (e[p_b] - e[n_b]); G[B + 2b] = c_b U_b; G[B + 2b + 1] = -c_b U_b
__global__ void __launch_bounds__(256) pool_pair_bwd_kernel(PoolArgs a, int32_t* status) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const float c = a.coef[b] * grad_scale(a.gscale, a.gscale_dev);
  const int64_t* tgt = a.rows + (int64_t)a.B * a.L + 2 * (int64_t)b;
  const f32x4* p = a.table + checked_id(tgt[0], a.n_table, status, lane == 0) * a.dv;
  const f32x4* n = a.table + checked_id(tgt[1], a.n_table, status, lane == 0) * a.dv;
  const f32x4* u = a.U + (int64_t)b * a.dv;
  f32x4* gh = a.G + (int64_t)b * a.dv;
  f32x4* gp = a.G + ((int64_t)a.B + 2 * (int64_t)b) * a.dv;
  for (int ch = lane; ch < a.dv; ch += 64) {
    const f32x4 uv = u[ch];
    gh[ch] = c * (p[ch] - n[ch]);
    gp[ch] = c * uv;
    gp[a.dv + ch] = -c * uv;
  }
}

static int pool_shape_ok(const char* who, int64_t n_table, int D, int B, int L) {
  PXR_REQUIRE(D > 0 && D % 4 == 0 && D <= 4096, "%s: need D %% 4 == 0 and 0 < D <= 4096 (D=%d)", who, D);
  PXR_REQUIRE(B > 0 && L >= 1 && (int64_t)B * (L + 2) < (1ll << 30), "%s: need B > 0, L >= 1 and B (L + 2) < 2^30 (B=%d, L=%d)", who,
              B, L);
  PXR_REQUIRE(n_table > 0 && n_table < (1ll << 40), "%s: bad table size %lld", who, (long long)n_table);
  return PXR_OK;
}

}  // namespace pxr

using namespace pxr;

extern "C" int pxr_pool_rows_f32(const float* table, int64_t n_table, int D, const int64_t* rows, int64_t pad_row, int B, int L,
                                 int mean, float* U, float* w, void* stream) {
  PXR_REQUIRE(table && rows && U && w, "pxr_pool_rows_f32: null pointer");
  if (int rc = pool_shape_ok("pxr_pool_rows_f32", n_table, D, B, L)) return rc;
  PXR_REQUIRE((((uintptr_t)table | (uintptr_t)U) & 15) == 0, "pxr_pool_rows_f32: table and U must be 16-byte aligned");
  PoolArgs a{};
  a.table = (const f32x4*)table; a.n_table = n_table; a.rows = rows; a.pad_row = pad_row; a.B = B; a.L = L; a.dv = D / 4;
  a.mean = mean != 0; a.U = (f32x4*)U; a.w = w;
  dispatch_ch<16>(a.dv, [&](auto ch) {
    hipLaunchKernelGGL(pool_rows_kernel<decltype(ch)::value>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a,
                       pxr_status_word());
  });
  return pxr_check_launch("pxr_pool_rows_f32");
}

extern "C" int pxr_pool_pair_fwd_f32(const float* table, int64_t n_table, int D, const int64_t* rows, int64_t pad_row, int B, int L,
                                     int mean, float* U, float* w, float* coef, float* lossrow, float* loss, void* stream) {
  PXR_REQUIRE(table && rows && U && w && coef && lossrow && loss, "pxr_pool_pair_fwd_f32: null pointer");
  if (int rc = pool_shape_ok("pxr_pool_pair_fwd_f32", n_table, D, B, L)) return rc;
  PXR_REQUIRE((((uintptr_t)table | (uintptr_t)U) & 15) == 0, "pxr_pool_pair_fwd_f32: table and U must be 16-byte aligned");
  PoolArgs a{};
  a.table = (const f32x4*)table; a.n_table = n_table; a.rows = rows; a.pad_row = pad_row; a.B = B; a.L = L; a.dv = D / 4;
  a.mean = mean != 0; a.U = (f32x4*)U; a.w = w; a.coef = coef; a.lossrow = lossrow;
  dispatch_ch<16>(a.dv, [&](auto ch) {
    hipLaunchKernelGGL(pool_pair_fwd_kernel<decltype(ch)::value>, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       a, pxr_status_word());
  });
  const int rc = pxr_check_launch("pxr_pool_pair_fwd_f32");
  if (rc) return rc;
  return pxr_bpr_loss_reduce(lossrow, B, 1, loss, stream);        // loss = (1/B) sum_b lossrow[b], fixed order
}

extern "C" int pxr_pool_pair_bwd_f32(const float* table, int64_t n_table, int D, const int64_t* rows, int B, int L, const float* U,
                                     const float* coef, float grad_scale, const float* grad_scale_dev, float* G, void* stream) {
  PXR_REQUIRE(table && rows && U && coef && G, "pxr_pool_pair_bwd_f32: null pointer");
  if (int rc = pool_shape_ok("pxr_pool_pair_bwd_f32", n_table, D, B, L)) return rc;
  PXR_REQUIRE((((uintptr_t)table | (uintptr_t)U | (uintptr_t)G) & 15) == 0, "pxr_pool_pair_bwd_f32: operands must be 16-byte aligned");
  PXR_REQUIRE(G != U, "pxr_pool_pair_bwd_f32: G must not alias U");
  PoolArgs a{};
  a.table = (const f32x4*)table; a.n_table = n_table; a.rows = rows; a.B = B; a.L = L; a.dv = D / 4; a.U = (f32x4*)U;
  a.coef = (float*)coef; a.gscale = grad_scale; a.gscale_dev = grad_scale_dev; a.G = (f32x4*)G;
  hipLaunchKernelGGL(pool_pair_bwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a, pxr_status_word());
  return pxr_check_launch("pxr_pool_pair_bwd_f32");
}
