// mf.hip -- MF (reference code/REC/model/IDNet/mf.py, MLPLayers of layers.py:239-294): the pair head over a users-then-items table
// with its gradient in sparse row form, and the towers' BatchNorm1d + tanh in training, backward and eval form.
//
// Table: one [1 + U + I, D] buffer, user u at row 1 + u, item i at row 1 + U + i.  Row 0 is a spare that nothing reads: the
// sparse-row machinery (embed_grad.hip, adamw.hip) treats id 0 as padding / an empty slot, and MF has no padding id.
//
// A step's occurrences are laid out as rows[3B] = [user row of b for b < B | item rows of item.view(-1): (i+_b, i-_b) for b < B],
// so the user tower reads rows[0:B] and the item tower rows[B:3B] in item.view(-1) order.  The sparse table gradient has one slot
// per occurrence, summed by pair_head.cuh's first-occurrence scheme: (row, sum) in the slot of a row's first occurrence, (0, zeros)
// -- the empty slot of a non-compacted list -- in the others.
#include "pair_head.cuh"

namespace pxr {

// Feature rows of sample b: the user's, the positive's and the negative's.  rows != NULL: rows of the table (ufeat == ifeat);
// rows == NULL: the towers' outputs, user b at ufeat row b, item j of item.view(-1) at ifeat row j.
struct MfPairArgs {
  const f32x4* ufeat;
  const f32x4* ifeat;
  const int64_t* rows;
  int hv, B;                   // H / 4; batch
  float* coef;                 // [B] d loss / d x_b
  float* lossrow;              // [B]
  float gscale;
  const float* gscale_dev;
  float eps;                   // the shift outside the log (forward): 1e-8 for mf.py, 0 for momf.py:59
  f32x4* du;                   // [B, hv]   (tower backward)
  f32x4* di;                   // [2B, hv]
};

__device__ __forceinline__ void mf_pair_rows_of(const MfPairArgs& a, int b, int64_t& ru, int64_t& rp, int64_t& rn) {
  if (a.rows) {
    ru = a.rows[b];
    rp = a.rows[a.B + 2 * (int64_t)b];
    rn = a.rows[a.B + 2 * (int64_t)b + 1];
  } else {
    ru = b;
    rp = 2 * (int64_t)b;
    rn = 2 * (int64_t)b + 1;
  }
}

// x_b = <u_b, i+_b> - <u_b, i-_b> into the tail with eps outside the log (mf.py forward: 1e-8).  One wave per b.
__global__ void __launch_bounds__(256) mf_pair_fwd_kernel(MfPairArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  int64_t ru, rp, rn;
  mf_pair_rows_of(a, b, ru, rp, rn);
  float sp, sn;
  pair_dots(a.ufeat + ru * a.hv, a.ifeat + rp * a.hv, a.ifeat + rn * a.hv, a.hv, lane, sp, sn);
  if (lane == 0) bpr_tail_log_outside(sp - sn, a.B, a.eps, a.lossrow[b], a.coef[b]);
}

// Tower form of the head's backward: d u_b = c_b (i+_b - i-_b), d i+_b = c_b u_b, d i-_b = -c_b u_b (dense, one wave per b).
__global__ void __launch_bounds__(256) mf_pair_bwd_kernel(MfPairArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const float c = a.coef[b] * a.gscale * (a.gscale_dev ? a.gscale_dev[0] : 1.f);
  const int64_t ru = b, rp = 2 * (int64_t)b, rn = rp + 1;
  for (int ch = lane; ch < a.hv; ch += 64) {
    const f32x4 u = a.ufeat[ru * a.hv + ch], p = a.ifeat[rp * a.hv + ch], n = a.ifeat[rn * a.hv + ch];
    a.du[ru * a.hv + ch] = c * (p - n);
    a.di[rp * a.hv + ch] = c * u;
    a.di[rn * a.hv + ch] = -c * u;
  }
}

// The step's table gradient as sparse rows, one wave per occurrence o of rows[3B].  Contribution of occurrence k = (b, t):
//   occ != NULL (towers): occ[k, :], the first layer's input gradient of that occurrence;
//   occ == NULL: the head's formula on the table rows (t = user: c_b (i+ - i-); positive: c_b u; negative: -c_b u).
struct MfTableGradArgs {
  const f32x4* table;
  const int64_t* rows;
  const float* coef;
  const f32x4* occ;
  int dv, B;
  float gscale;
  const float* gscale_dev;
  int64_t* sp_idx;             // [3B]
  f32x4* sp_rows;              // [3B, dv]
  int32_t* sp_n;
};

template <int CH>
__global__ void __launch_bounds__(256) mf_table_grad_kernel(MfTableGradArgs a) {
  const int lane = threadIdx.x & 63;
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n_occ = 3 * a.B;
  if (o == 0 && lane == 0) a.sp_n[0] = n_occ;
  if (o >= n_occ) return;
  const int64_t node = a.rows[o];
  const bool first = is_first_occurrence(a.rows, 0, o, node, lane);
  f32x4 s[CH];
  row_zero(s);
  if (first) {
    const float g = grad_scale(a.gscale, a.gscale_dev);
    for_each_occurrence(a.rows, o, n_occ, node, lane, [&](int kk) {
      if (a.occ) {
        row_add_scaled(s, 1.f, a.occ + (int64_t)kk * a.dv, a.dv, lane);      // 1 x is x: the plain sum of the occurrences' rows
        return;
      }
      const bool is_user = kk < a.B;
      const int b = is_user ? kk : (kk - a.B) >> 1;
      const float c = a.coef[b] * g;
      if (is_user)
        row_add_scaled_diff(s, c, a.table + a.rows[a.B + 2 * (int64_t)b] * a.dv, a.table + a.rows[a.B + 2 * (int64_t)b + 1] * a.dv,
                            a.dv, lane);
      else
        row_add_scaled(s, ((kk - a.B) & 1) ? -c : c, a.table + a.rows[b] * a.dv, a.dv, lane);
    });
  }
  row_store(s, a.sp_rows + (int64_t)o * a.dv, a.dv, lane);
  if (lane == 0) a.sp_idx[o] = first ? node : 0;
}

// MOMF (momf.py): the same occurrence list over TWO row spaces -- rows[0:B] are rows of the user table, rows[B:3B] positions into
// the encoder's output E [M, D] -- and two sinks.  Occurrence o < B is mf_table_grad_kernel's user slot: (row, sum) at the first
// occurrence of a user row, (0, zeros) at the others, scanned within rows[0:B].  Occurrence o >= B is scanned within rows[B:3B];
// the first occurrence of position m stores its sum into dE[m, :] (zeroed by the entry before the launch) and the later ones write
// nothing.  Contributions and their order are mf_table_grad_kernel's, so both sinks carry its bits.
struct MomfGradArgs {
  const f32x4* utable;         // [n_utable, dv]
  const f32x4* E;              // [M, dv]
  const int64_t* rows;         // [3B] = [user rows | positions (positive, negative) of b]
  const float* coef;
  const f32x4* occ;            // [3B, dv] | NULL
  int dv, B;
  int64_t M;
  float gscale;
  const float* gscale_dev;
  int64_t* sp_idx;             // [B]
  f32x4* sp_rows;              // [B, dv]
  int32_t* sp_n;
  f32x4* dE;                   // [M, dv]
};

template <int CH>
__global__ void __launch_bounds__(256) momf_pair_grad_kernel(MomfGradArgs a) {
  const int lane = threadIdx.x & 63;
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n_occ = 3 * a.B;
  if (o == 0 && lane == 0) a.sp_n[0] = a.B;
  if (o >= n_occ) return;
  const bool user_sink = o < a.B;
  const int lo = user_sink ? 0 : a.B, hi = user_sink ? a.B : n_occ;
  const int64_t node = a.rows[o];
  const bool first = is_first_occurrence(a.rows, lo, o, node, lane);
  if (!first && !user_sink) return;                  // a later occurrence of a position: its sum is the first one's
  f32x4 s[CH];
  row_zero(s);
  if (first) {
    const float g = grad_scale(a.gscale, a.gscale_dev);
    for_each_occurrence(a.rows, o, hi, node, lane, [&](int kk) {
      if (a.occ) {
        row_add_scaled(s, 1.f, a.occ + (int64_t)kk * a.dv, a.dv, lane);      // 1 x is x: the plain sum of the occurrences' rows
        return;
      }
      const int b = user_sink ? kk : (kk - a.B) >> 1;
      const float c = a.coef[b] * g;
      if (user_sink)
        row_add_scaled_diff(s, c, a.E + a.rows[a.B + 2 * (int64_t)b] * a.dv, a.E + a.rows[a.B + 2 * (int64_t)b + 1] * a.dv, a.dv,
                            lane);
      else
        row_add_scaled(s, ((kk - a.B) & 1) ? -c : c, a.utable + a.rows[b] * a.dv, a.dv, lane);
    });
  }
  if (user_sink) {
    row_store(s, a.sp_rows + (int64_t)o * a.dv, a.dv, lane);
    if (lane == 0) a.sp_idx[o] = first ? node : 0;
  } else if (node >= 0 && node < a.M) {              // (the row list is checked and clamped upstream: never false there)
    row_store(s, a.dE + node * a.dv, a.dv, lane);
  }
}

// ---------------------------------------------------------------- BatchNorm1d + tanh over x [R, H] (MLPLayers: Linear -> BN -> Tanh)
// A workgroup owns BN_CC float4 columns and walks every row with BN_RL row lanes; the BN_RL partial sums of a column are added in
// lane order through LDS, so each column statistic has one fixed summation order (bit-identical from run to run).
constexpr int BN_CC = 8, BN_RL = 32;

struct BnArgs {
  const f32x4* x;              // [R, hv] (the Linear output)
  const f32x4* y;              // [R, hv] (the tanh output: backward)
  const f32x4* dy;             // [R, hv]
  f32x4* out;                  // y (forward / eval) or dx (backward)
  const float* gamma;
  const float* beta;
  float* mean;                 // [H] batch mean (saved by the forward, read by the backward)
  float* rstd;                 // [H] 1 / sqrt(biased var + eps)
  float* run_mean;
  float* run_var;
  int64_t* n_tracked;
  float* dgamma;
  float* dbeta;
  int R, hv;
  float eps, momentum;
};

__device__ __forceinline__ f32x4 bn_col_reduce(f32x4 s, f32x4 (*red)[BN_CC], int rl, int cc) {
  __syncthreads();                                   // red may still be read by the previous reduction
  red[rl][cc] = s;
  __syncthreads();
  f32x4 t = red[0][cc];
#pragma unroll
  for (int k = 1; k < BN_RL; ++k) t += red[k][cc];
  return t;
}

__device__ __forceinline__ f32x4 ld4(const float* p, int c4) { return reinterpret_cast<const f32x4*>(p)[c4]; }

__device__ __forceinline__ f32x4 tanh4(const f32x4& z) { return f32x4{tanhf(z.x), tanhf(z.y), tanhf(z.z), tanhf(z.w)}; }

// training forward: batch statistics (mean, then the centred sum of squares), y = tanh(gamma xhat + beta), running statistics
// updated with the unbiased variance, num_batches_tracked += 1
__global__ void __launch_bounds__(256) mf_bn_tanh_fwd_kernel(BnArgs a) {
  __shared__ f32x4 red[BN_RL][BN_CC];
  const int cc = threadIdx.x % BN_CC, rl = threadIdx.x / BN_CC;
  const int c4 = blockIdx.x * BN_CC + cc;
  const bool ok = c4 < a.hv;
  const float inv_r = 1.f / (float)a.R;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (ok)
    for (int r = rl; r < a.R; r += BN_RL) s += a.x[(int64_t)r * a.hv + c4];
  const f32x4 mean = bn_col_reduce(s, red, rl, cc) * inv_r;
  s = f32x4{0.f, 0.f, 0.f, 0.f};
  if (ok)
    for (int r = rl; r < a.R; r += BN_RL) {
      const f32x4 d = a.x[(int64_t)r * a.hv + c4] - mean;
      s += d * d;
    }
  const f32x4 ss = bn_col_reduce(s, red, rl, cc);
  const f32x4 var = ss * inv_r;
  const f32x4 rstd = f32x4{1.f / sqrtf(var.x + a.eps), 1.f / sqrtf(var.y + a.eps), 1.f / sqrtf(var.z + a.eps),
                       1.f / sqrtf(var.w + a.eps)};
  if (!ok) return;
  if (rl == 0) {
    reinterpret_cast<f32x4*>(a.mean)[c4] = mean;
    reinterpret_cast<f32x4*>(a.rstd)[c4] = rstd;
    const float mo = a.momentum;
    const f32x4 uvar = ss * (1.f / (float)(a.R - 1));
    f32x4* rm = reinterpret_cast<f32x4*>(a.run_mean) + c4;
    f32x4* rv = reinterpret_cast<f32x4*>(a.run_var) + c4;
    *rm = (1.f - mo) * *rm + mo * mean;
    *rv = (1.f - mo) * *rv + mo * uvar;
    if (c4 == 0 && a.n_tracked) a.n_tracked[0] += 1;
  }
  const f32x4 g = ld4(a.gamma, c4) * rstd, bt = ld4(a.beta, c4);
  for (int r = rl; r < a.R; r += BN_RL) {
    const int64_t o = (int64_t)r * a.hv + c4;
    a.out[o] = tanh4((a.x[o] - mean) * g + bt);
  }
}

// backward through tanh and the batch normalisation: dz = dy (1 - y^2), dbeta = sum dz, dgamma = sum dz xhat,
// dx = gamma rstd / R (R dz - dbeta - xhat dgamma)
__global__ void __launch_bounds__(256) mf_bn_tanh_bwd_kernel(BnArgs a) {
  __shared__ f32x4 red[BN_RL][BN_CC];
  const int cc = threadIdx.x % BN_CC, rl = threadIdx.x / BN_CC;
  const int c4 = blockIdx.x * BN_CC + cc;
  const bool ok = c4 < a.hv;
  const f32x4 mean = ok ? ld4(a.mean, c4) : f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 rstd = ok ? ld4(a.rstd, c4) : f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 s1 = f32x4{0.f, 0.f, 0.f, 0.f}, s2 = s1;
  if (ok)
    for (int r = rl; r < a.R; r += BN_RL) {
      const int64_t o = (int64_t)r * a.hv + c4;
      const f32x4 y = a.y[o];
      const f32x4 dz = a.dy[o] * (1.f - y * y);
      s1 += dz;
      s2 += dz * ((a.x[o] - mean) * rstd);
    }
  const f32x4 db = bn_col_reduce(s1, red, rl, cc);
  const f32x4 dg = bn_col_reduce(s2, red, rl, cc);
  if (!ok) return;
  if (rl == 0) {
    reinterpret_cast<f32x4*>(a.dbeta)[c4] = db;
    reinterpret_cast<f32x4*>(a.dgamma)[c4] = dg;
  }
  const float fr = (float)a.R;
  const f32x4 k = ld4(a.gamma, c4) * rstd * (1.f / fr);
  for (int r = rl; r < a.R; r += BN_RL) {
    const int64_t o = (int64_t)r * a.hv + c4;
    const f32x4 y = a.y[o];
    const f32x4 dz = a.dy[o] * (1.f - y * y);
    const f32x4 xh = (a.x[o] - mean) * rstd;
    a.out[o] = k * (fr * dz - db - xh * dg);
  }
}

// eval: y = tanh(gamma (x - running_mean) / sqrt(running_var + eps) + beta), elementwise (grid-stride over float4s)
__global__ void __launch_bounds__(256) mf_bn_tanh_eval_kernel(BnArgs a) {
  const int64_t n = (int64_t)a.R * a.hv;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int c4 = (int)(e % a.hv);
    const f32x4 rv = ld4(a.run_var, c4);
    const f32x4 rs = f32x4{1.f / sqrtf(rv.x + a.eps), 1.f / sqrtf(rv.y + a.eps), 1.f / sqrtf(rv.z + a.eps), 1.f / sqrtf(rv.w + a.eps)};
    a.out[e] = tanh4((a.x[e] - ld4(a.run_mean, c4)) * (ld4(a.gamma, c4) * rs) + ld4(a.beta, c4));
  }
}

}  // namespace pxr

using namespace pxr;

extern "C" int pxr_mf_pair_fwd_eps_f32(const float* ufeat, const float* ifeat, const int64_t* rows, int H, int B, float eps,
                                       float* coef, float* lossrow, float* loss, void* stream) {
  PXR_REQUIRE(ufeat && ifeat && coef && lossrow && loss, "pxr_mf_pair_fwd_eps_f32: null pointer");
  PXR_REQUIRE(H > 0 && H % 4 == 0 && H <= 4096, "pxr_mf_pair_fwd_eps_f32: need H %% 4 == 0 and 0 < H <= 4096 (H=%d)", H);
  PXR_REQUIRE(B > 0 && B <= (1 << 28), "pxr_mf_pair_fwd_eps_f32: bad batch size %d", B);
  PXR_REQUIRE(eps >= 0.f && eps < INFINITY, "pxr_mf_pair_fwd_eps_f32: eps must be finite and >= 0");
  PXR_REQUIRE((((uintptr_t)ufeat | (uintptr_t)ifeat) & 15) == 0, "pxr_mf_pair_fwd_eps_f32: features must be 16-byte aligned");
  MfPairArgs a{};
  a.ufeat = (const f32x4*)ufeat; a.ifeat = (const f32x4*)ifeat; a.rows = rows; a.hv = H / 4; a.B = B;
  a.coef = coef; a.lossrow = lossrow; a.eps = eps;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mf_pair_fwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, a);
  const int rc = pxr_check_launch("pxr_mf_pair_fwd_eps_f32");
  if (rc) return rc;
  return pxr_bpr_loss_reduce(lossrow, B, 1, loss, stream);        // loss = (1/B) sum_b lossrow[b], fixed order
}

extern "C" int pxr_mf_pair_fwd_f32(const float* ufeat, const float* ifeat, const int64_t* rows, int H, int B, float* coef,
                                   float* lossrow, float* loss, void* stream) {
  return pxr_mf_pair_fwd_eps_f32(ufeat, ifeat, rows, H, B, 1e-8f, coef, lossrow, loss, stream);
}

extern "C" int pxr_mf_pair_bwd_f32(const float* ufeat, const float* ifeat, const float* coef, int H, int B, float grad_scale,
                                   const float* grad_scale_dev, float* du, float* di, void* stream) {
  PXR_REQUIRE(ufeat && ifeat && coef && du && di, "pxr_mf_pair_bwd_f32: null pointer");
  PXR_REQUIRE(H > 0 && H % 4 == 0 && H <= 4096, "pxr_mf_pair_bwd_f32: need H %% 4 == 0 and 0 < H <= 4096 (H=%d)", H);
  PXR_REQUIRE(B > 0 && B <= (1 << 28), "pxr_mf_pair_bwd_f32: bad batch size %d", B);
  PXR_REQUIRE((((uintptr_t)ufeat | (uintptr_t)ifeat | (uintptr_t)du | (uintptr_t)di) & 15) == 0,
              "pxr_mf_pair_bwd_f32: operands must be 16-byte aligned");
  MfPairArgs a{};
  a.ufeat = (const f32x4*)ufeat; a.ifeat = (const f32x4*)ifeat; a.hv = H / 4; a.B = B; a.coef = (float*)coef;
  a.gscale = grad_scale; a.gscale_dev = grad_scale_dev; a.du = (f32x4*)du; a.di = (f32x4*)di;
  hipLaunchKernelGGL(mf_pair_bwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  return pxr_check_launch("pxr_mf_pair_bwd_f32");
}

extern "C" int pxr_mf_table_grad_f32(const float* table, int64_t n_table, int D, const int64_t* rows, int B, const float* coef,
                                     const float* occ, float grad_scale, const float* grad_scale_dev, int64_t* sp_idx,
                                     float* sp_rows, int32_t* sp_n, int64_t cap, void* stream) {
  PXR_REQUIRE(rows && sp_idx && sp_rows && sp_n, "pxr_mf_table_grad_f32: null pointer");
  PXR_REQUIRE(occ || (table && coef), "pxr_mf_table_grad_f32: need occ, or table and coef");
  PXR_REQUIRE(D > 0 && D % 4 == 0 && D <= 4096, "pxr_mf_table_grad_f32: need D %% 4 == 0 and 0 < D <= 4096 (D=%d)", D);
  PXR_REQUIRE(B > 0 && B <= (1 << 28) / 3, "pxr_mf_table_grad_f32: bad batch size %d", B);
  PXR_REQUIRE(cap >= 3 * (int64_t)B, "pxr_mf_table_grad_f32: sparse capacity %lld < 3B = %lld", (long long)cap,
              3 * (long long)B);
  PXR_REQUIRE(occ || n_table > 1, "pxr_mf_table_grad_f32: bad table size");
  MfTableGradArgs a{};
  a.table = (const f32x4*)table; a.rows = rows; a.coef = coef; a.occ = (const f32x4*)occ; a.dv = D / 4; a.B = B;
  a.gscale = grad_scale; a.gscale_dev = grad_scale_dev; a.sp_idx = sp_idx; a.sp_rows = (f32x4*)sp_rows; a.sp_n = sp_n;
  dispatch_ch<16>(a.dv, [&](auto ch) {
    hipLaunchKernelGGL(mf_table_grad_kernel<decltype(ch)::value>, dim3((unsigned)((3 * B + 3) / 4)), dim3(256), 0,
                       (hipStream_t)stream, a);
  });
  return pxr_check_launch("pxr_mf_table_grad_f32");
}

extern "C" int pxr_momf_pair_grad_f32(const float* utable, int64_t n_utable, const float* E, int64_t M, int D, const int64_t* rows,
                                      int B, const float* coef, const float* occ, float grad_scale, const float* grad_scale_dev,
                                      int64_t* sp_idx, float* sp_rows, int32_t* sp_n, int64_t cap, float* dE, void* stream) {
  PXR_REQUIRE(rows && sp_idx && sp_rows && sp_n && dE, "pxr_momf_pair_grad_f32: null pointer");
  PXR_REQUIRE(occ || (utable && E && coef), "pxr_momf_pair_grad_f32: need occ, or utable, E and coef");
  PXR_REQUIRE(D > 0 && D % 4 == 0 && D <= 4096, "pxr_momf_pair_grad_f32: need D %% 4 == 0 and 0 < D <= 4096 (D=%d)", D);
  PXR_REQUIRE(B > 0 && B <= (1 << 28) / 3, "pxr_momf_pair_grad_f32: bad batch size %d", B);
  PXR_REQUIRE(cap >= (int64_t)B, "pxr_momf_pair_grad_f32: sparse capacity %lld < B = %d", (long long)cap, B);
  PXR_REQUIRE(M > 0 && M < (1ll << 40), "pxr_momf_pair_grad_f32: bad number of encoder rows %lld", (long long)M);
  PXR_REQUIRE(occ || n_utable > 1, "pxr_momf_pair_grad_f32: bad user table size");
  PXR_REQUIRE((((uintptr_t)utable | (uintptr_t)E | (uintptr_t)occ | (uintptr_t)sp_rows | (uintptr_t)dE) & 15) == 0,
              "pxr_momf_pair_grad_f32: operands must be 16-byte aligned");
  PXR_REQUIRE(dE != E && dE != occ && dE != utable && dE != sp_rows, "pxr_momf_pair_grad_f32: dE must not alias an operand");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(dE, 0, (size_t)M * (size_t)D * sizeof(float), st) != hipSuccess) {      // rows nobody reads: +0.0
    pxr_set_error("pxr_momf_pair_grad_f32: memset failed");
    return PXR_ERR_LAUNCH;
  }
  MomfGradArgs a{};
  a.utable = (const f32x4*)utable; a.E = (const f32x4*)E; a.rows = rows; a.coef = coef; a.occ = (const f32x4*)occ;
  a.dv = D / 4; a.B = B; a.M = M; a.gscale = grad_scale; a.gscale_dev = grad_scale_dev;
  a.sp_idx = sp_idx; a.sp_rows = (f32x4*)sp_rows; a.sp_n = sp_n; a.dE = (f32x4*)dE;
  dispatch_ch<16>(a.dv, [&](auto ch) {
    hipLaunchKernelGGL(momf_pair_grad_kernel<decltype(ch)::value>, dim3((unsigned)((3 * B + 3) / 4)), dim3(256), 0, st, a);
  });
  return pxr_check_launch("pxr_momf_pair_grad_f32");
}

static int mf_bn_shape_ok(const char* who, int R, int H) {
  PXR_REQUIRE(R > 0 && H > 0 && H % 4 == 0 && H <= 4096, "%s: need R > 0 and H %% 4 == 0, 0 < H <= 4096 (R=%d, H=%d)", who, R, H);
  return PXR_OK;
}

extern "C" int pxr_mf_bn_tanh_fwd_f32(const float* x, int R, int H, const float* gamma, const float* beta, float eps, float momentum,
                                      float* running_mean, float* running_var, int64_t* num_batches_tracked, float* y,
                                      float* mean, float* rstd, void* stream) {
  PXR_REQUIRE(x && gamma && beta && running_mean && running_var && y && mean && rstd, "pxr_mf_bn_tanh_fwd_f32: null pointer");
  if (int rc = mf_bn_shape_ok("pxr_mf_bn_tanh_fwd_f32", R, H)) return rc;
  PXR_REQUIRE(R >= 2, "pxr_mf_bn_tanh_fwd_f32: training statistics need more than one row (R=%d)", R);
  PXR_REQUIRE(x != y, "pxr_mf_bn_tanh_fwd_f32: y must not alias x (the backward reads both)");
  BnArgs a{};
  a.x = (const f32x4*)x; a.out = (f32x4*)y; a.gamma = gamma; a.beta = beta; a.mean = mean; a.rstd = rstd;
  a.run_mean = running_mean; a.run_var = running_var; a.n_tracked = num_batches_tracked; a.R = R; a.hv = H / 4;
  a.eps = eps; a.momentum = momentum;
  const int hv = H / 4;
  hipLaunchKernelGGL(mf_bn_tanh_fwd_kernel, dim3((unsigned)((hv + BN_CC - 1) / BN_CC)), dim3(256), 0, (hipStream_t)stream, a);
  return pxr_check_launch("pxr_mf_bn_tanh_fwd_f32");
}

extern "C" int pxr_mf_bn_tanh_bwd_f32(const float* dy, const float* x, const float* y, const float* mean, const float* rstd,
                                      const float* gamma, int R, int H, float* dx, float* dgamma, float* dbeta, void* stream) {
  PXR_REQUIRE(dy && x && y && mean && rstd && gamma && dx && dgamma && dbeta, "pxr_mf_bn_tanh_bwd_f32: null pointer");
  if (int rc = mf_bn_shape_ok("pxr_mf_bn_tanh_bwd_f32", R, H)) return rc;
  PXR_REQUIRE(dx != dy && dx != x && dx != y, "pxr_mf_bn_tanh_bwd_f32: dx must not alias an input (columns are read twice)");
  BnArgs a{};
  a.x = (const f32x4*)x; a.y = (const f32x4*)y; a.dy = (const f32x4*)dy; a.out = (f32x4*)dx; a.gamma = gamma;
  a.mean = (float*)mean; a.rstd = (float*)rstd; a.dgamma = dgamma; a.dbeta = dbeta; a.R = R; a.hv = H / 4;
  const int hv = H / 4;
  hipLaunchKernelGGL(mf_bn_tanh_bwd_kernel, dim3((unsigned)((hv + BN_CC - 1) / BN_CC)), dim3(256), 0, (hipStream_t)stream, a);
  return pxr_check_launch("pxr_mf_bn_tanh_bwd_f32");
}

extern "C" int pxr_mf_bn_tanh_eval_f32(const float* x, int64_t R, int H, const float* gamma, const float* beta,
                                       const float* running_mean, const float* running_var, float eps, float* y, void* stream) {
  PXR_REQUIRE(x && gamma && beta && running_mean && running_var && y, "pxr_mf_bn_tanh_eval_f32: null pointer");
  PXR_REQUIRE(R > 0 && R < (1ll << 31) && H > 0 && H % 4 == 0 && H <= 4096,
              "pxr_mf_bn_tanh_eval_f32: need 0 < R < 2^31 and H %% 4 == 0, 0 < H <= 4096 (H=%d)", H);
  BnArgs a{};
  a.x = (const f32x4*)x; a.out = (f32x4*)y; a.gamma = gamma; a.beta = beta; a.run_mean = (float*)running_mean;
  a.run_var = (float*)running_var; a.R = (int)R; a.hv = H / 4; a.eps = eps;
  int64_t blocks = (R * (H / 4) + 255) / 256;
  if (blocks > 256 * 64) blocks = 256 * 64;
  hipLaunchKernelGGL(mf_bn_tanh_eval_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  return pxr_check_launch("pxr_mf_bn_tanh_eval_f32");
}
