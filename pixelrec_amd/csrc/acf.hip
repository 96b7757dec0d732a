// acf.hip -- ACF (reference code/REC/model/ViNet/acf.py): the two attention levels of the user net.
//
//   region level (ACFFeatureNet.forward), per history occurrence r = (b, p) with H regions x[r, h, :]:
//     s_h = <w, relu(x~[r, h, :] + u~[b, :])>     beta = softmax_H(s)     pooled[r, :] = mask_r sum_h beta_h x[r, h, :]
//   item level (ACFUserNet.forward), per user b with P history items:
//     t_p = <w, relu(uw[b, :] + pq[r, :] + cx[r, :])>     alpha = softmax_P(t) over the unmasked p (all masked: alpha = 0)
//     user[b, :] = uw[b, :] + sum_p alpha_p prof[r, :]
// mask_r = (profile id of r != 0).  The scalar biases of the two `w` Linears are constant along the softmax axis and are not read.
//
// Table: one [1 + I + U, E] buffer, item i at row 1 + i (item 0 is the reference's padding row: read, never given a gradient),
// user u at row 1 + I + u, row 0 a spare nothing reads (the sparse-row machinery treats id 0 as an empty slot).
//
// One workgroup (4 waves) per r (region level) or per b (item level): a wave owns one h (or p) at a time for the inner products,
// then every thread owns float4 columns for the weighted sums.  Every sum has one fixed order; no atomics on floats.
#include "pair_head.cuh"

namespace pxr {

__device__ __forceinline__ f32x4 acf_relu4(const f32x4& z) {
  return f32x4{fmaxf(z.x, 0.f), fmaxf(z.y, 0.f), fmaxf(z.z, 0.f), fmaxf(z.w, 0.f)};
}
__device__ __forceinline__ f32x4 acf_step4(const f32x4& z) {
  return f32x4{z.x > 0.f ? 1.f : 0.f, z.y > 0.f ? 1.f : 0.f, z.z > 0.f ? 1.f : 0.f, z.w > 0.f ? 1.f : 0.f};
}
constexpr int ACF_MAX_N = 1024;      // regions per item / history items per user held in LDS

// softmax over s[0..n) held in LDS, computed by every thread alike (one fixed order): returns max and 1 / sum
__device__ __forceinline__ void acf_softmax_stats(const float* s, int n, float& mx, float& inv) {
  mx = -INFINITY;
  for (int k = 0; k < n; ++k) mx = fmaxf(mx, s[k]);
  float sum = 0.f;
  if (mx > -INFINITY)
    for (int k = 0; k < n; ++k) sum += expf(s[k] - mx);
  inv = sum > 0.f ? 1.f / sum : 0.f;          // every entry masked: all weights 0 (the reference turns its NaN into 0)
}

struct AcfRegionArgs {
  const f32x4* x;              // [R, H, ev]
  const f32x4* xt;             // [R, H, ev]
  const f32x4* ut;             // [B, ev]
  const f32x4* w;              // [ev]
  const int64_t* profile;      // [R] item ids (0 = padding)
  float* beta;                 // [R, H]
  f32x4* pooled;               // [R, ev]
  const f32x4* dpooled;        // [R, ev]    (backward)
  f32x4* dxt;                  // [R, H, ev]
  f32x4* dutp;                 // [R, ev]: sum_h dxt[r, h, :]
  f32x4* dwp;                  // [R, ev]: sum_h ds_h relu(z_h)
  int R, P, H, ev;
};

template <int CH>
__global__ void __launch_bounds__(256) acf_region_fwd_kernel(AcfRegionArgs a) {
  __shared__ float s[ACF_MAX_N];
  const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = r / a.P;
  if (a.profile[r] == 0) {                   // masked: pooled = 0, and beta = 0 makes the backward of this r vanish
    for (int h = threadIdx.x; h < a.H; h += 256) a.beta[(int64_t)r * a.H + h] = 0.f;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int c = threadIdx.x + k * 256;
      if (c < a.ev) a.pooled[(int64_t)r * a.ev + c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    return;
  }
  const f32x4* ut = a.ut + (int64_t)b * a.ev;
  for (int h = wave; h < a.H; h += 4) {
    const f32x4* xt = a.xt + ((int64_t)r * a.H + h) * a.ev;
    float acc = 0.f;
    for (int c = lane; c < a.ev; c += 64) acc += dot4(a.w[c], acf_relu4(xt[c] + ut[c]));
    acc = wave_sum(acc);
    if (lane == 0) s[h] = acc;
  }
  __syncthreads();
  float mx, inv;
  acf_softmax_stats(s, a.H, mx, inv);
  for (int h = threadIdx.x; h < a.H; h += 256) a.beta[(int64_t)r * a.H + h] = expf(s[h] - mx) * inv;
  f32x4 acc[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int h = 0; h < a.H; ++h) {
    const float bh = expf(s[h] - mx) * inv;
    const f32x4* x = a.x + ((int64_t)r * a.H + h) * a.ev;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int c = threadIdx.x + k * 256;
      if (c < a.ev) acc[k] += bh * x[c];
    }
  }
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int c = threadIdx.x + k * 256;
    if (c < a.ev) a.pooled[(int64_t)r * a.ev + c] = acc[k];
  }
}

// backward from dpooled: d beta_h = <mask dpooled, x_h>, ds = softmax backward, dxt[r, h, :] = ds_h w (z_h > 0) with z = x~ + u~
template <int CH>
__global__ void __launch_bounds__(256) acf_region_bwd_kernel(AcfRegionArgs a) {
  __shared__ float ds[ACF_MAX_N];
  const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = r / a.P;
  const bool masked = a.profile[r] == 0;
  const float* beta = a.beta + (int64_t)r * a.H;
  if (!masked) {
    const f32x4* dp = a.dpooled + (int64_t)r * a.ev;
    for (int h = wave; h < a.H; h += 4) {
      const f32x4* x = a.x + ((int64_t)r * a.H + h) * a.ev;
      float acc = 0.f;
      for (int c = lane; c < a.ev; c += 64) acc += dot4(dp[c], x[c]);
      acc = wave_sum(acc);
      if (lane == 0) ds[h] = acc;
    }
  }
  __syncthreads();
  float dot = 0.f;
  if (!masked)
    for (int h = 0; h < a.H; ++h) dot += beta[h] * ds[h];
  __syncthreads();
  for (int h = threadIdx.x; h < a.H; h += 256) ds[h] = masked ? 0.f : beta[h] * (ds[h] - dot);
  __syncthreads();
  const f32x4* ut = a.ut + (int64_t)b * a.ev;
  f32x4 su[CH], sw[CH], uu[CH], ww[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int c = threadIdx.x + k * 256;
    su[k] = sw[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    uu[k] = c < a.ev ? ut[c] : su[k];
    ww[k] = c < a.ev ? a.w[c] : su[k];
  }
  for (int h = 0; h < a.H; ++h) {
    const float d = ds[h];
    const int64_t o = ((int64_t)r * a.H + h) * a.ev;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int c = threadIdx.x + k * 256;
      if (c < a.ev) {
        f32x4 dz = f32x4{0.f, 0.f, 0.f, 0.f};
        if (!masked) {
          const f32x4 z = a.xt[o + c] + uu[k];
          dz = d * ww[k] * acf_step4(z);
          su[k] += dz;
          sw[k] += d * acf_relu4(z);
        }
        a.dxt[o + c] = dz;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int c = threadIdx.x + k * 256;
    if (c < a.ev) {
      a.dutp[(int64_t)r * a.ev + c] = su[k];
      a.dwp[(int64_t)r * a.ev + c] = sw[k];
    }
  }
}

// out[b, :] = sum_p in[b, p, :] in ascending p (float4 columns)
__global__ void __launch_bounds__(256) acf_group_sum_kernel(const f32x4* __restrict__ in, f32x4* __restrict__ out, int B, int P, int ev) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)B * ev) return;
  const int b = (int)(e / ev), c = (int)(e % ev);
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < P; ++p) s += in[((int64_t)b * P + p) * ev + c];
  out[e] = s;
}

// dx[r, h, :] = (dx[r, h, :] + beta[r, h] dpooled[r, :]) (x[r, h, :] > 0): the pooled path joins the feats.w_x input gradient
// already in dx, and the ReLU of dim_reductor is applied (beta = 0 on a masked r)
__global__ void __launch_bounds__(256) acf_region_dx_kernel(f32x4* __restrict__ dx, const f32x4* __restrict__ x,
                                                             const float* __restrict__ beta, const f32x4* __restrict__ dpooled,
                                                             int64_t n_rows, int H, int ev) {
  const int64_t total = n_rows * ev;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t row = e / ev;
    const int c = (int)(e - row * ev);
    const int64_t r = row / H;
    dx[e] = (dx[e] + beta[row] * dpooled[r * ev + c]) * acf_step4(x[e]);
  }
}

struct AcfItemArgs {
  const f32x4* uw;             // [B, ev]
  const f32x4* pq;             // [R, ev]
  const f32x4* cx;             // [R, ev]
  const f32x4* prof;           // [R, ev]
  const f32x4* w;              // [ev]
  const int64_t* profile;      // [R]
  float* alpha;                // [B, P]
  f32x4* user;                 // [B, ev]
  const f32x4* duser;          // [B, ev]   (backward)
  f32x4* da;                   // [R, ev]: gradient of the pre-activation (the same for pq and cx)
  f32x4* dprof;                // [R, ev]: alpha_p duser (the direct path onto the profile rows)
  f32x4* duw;                  // [B, ev]: duser + sum_p da
  f32x4* dwp;                  // [B, ev]: sum_p dt_p relu(a_p)
  int B, P, ev;
};

template <int CH>
__global__ void __launch_bounds__(256) acf_item_fwd_kernel(AcfItemArgs a) {
  __shared__ float t[ACF_MAX_N];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const f32x4* uw = a.uw + (int64_t)b * a.ev;
  for (int p = wave; p < a.P; p += 4) {
    const int64_t r = (int64_t)b * a.P + p;
    float acc = 0.f;
    for (int c = lane; c < a.ev; c += 64) acc += dot4(a.w[c], acf_relu4(uw[c] + a.pq[r * a.ev + c] + a.cx[r * a.ev + c]));
    acc = wave_sum(acc);
    if (lane == 0) t[p] = a.profile[r] == 0 ? -INFINITY : acc;
  }
  __syncthreads();
  float mx, inv;
  acf_softmax_stats(t, a.P, mx, inv);
  for (int p = threadIdx.x; p < a.P; p += 256) a.alpha[(int64_t)b * a.P + p] = inv > 0.f ? expf(t[p] - mx) * inv : 0.f;
  f32x4 acc[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int c = threadIdx.x + k * 256;
    acc[k] = c < a.ev ? uw[c] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int p = 0; p < a.P; ++p) {
    const float al = inv > 0.f ? expf(t[p] - mx) * inv : 0.f;
    if (al == 0.f) continue;                 // (uniform over the workgroup)
    const f32x4* pr = a.prof + ((int64_t)b * a.P + p) * a.ev;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int c = threadIdx.x + k * 256;
      if (c < a.ev) acc[k] += al * pr[c];
    }
  }
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int c = threadIdx.x + k * 256;
    if (c < a.ev) a.user[(int64_t)b * a.ev + c] = acc[k];
  }
}

template <int CH>
__global__ void __launch_bounds__(256) acf_item_bwd_kernel(AcfItemArgs a) {
  __shared__ float dt[ACF_MAX_N];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const f32x4* du = a.duser + (int64_t)b * a.ev;
  const float* alpha = a.alpha + (int64_t)b * a.P;
  for (int p = wave; p < a.P; p += 4) {
    const f32x4* pr = a.prof + ((int64_t)b * a.P + p) * a.ev;
    float acc = 0.f;
    for (int c = lane; c < a.ev; c += 64) acc += dot4(du[c], pr[c]);
    acc = wave_sum(acc);
    if (lane == 0) dt[p] = acc;
  }
  __syncthreads();
  float dot = 0.f;
  for (int p = 0; p < a.P; ++p) dot += alpha[p] * dt[p];
  __syncthreads();
  for (int p = threadIdx.x; p < a.P; p += 256) dt[p] = alpha[p] * (dt[p] - dot);
  __syncthreads();
  const f32x4* uw = a.uw + (int64_t)b * a.ev;
  f32x4 su[CH], sw[CH], uu[CH], ww[CH], dd[CH];
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int c = threadIdx.x + k * 256;
    su[k] = sw[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    uu[k] = c < a.ev ? uw[c] : su[k];
    ww[k] = c < a.ev ? a.w[c] : su[k];
    dd[k] = c < a.ev ? du[c] : su[k];
  }
  for (int p = 0; p < a.P; ++p) {
    const float d = dt[p], al = alpha[p];
    const int64_t o = ((int64_t)b * a.P + p) * a.ev;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int c = threadIdx.x + k * 256;
      if (c < a.ev) {
        const f32x4 z = uu[k] + a.pq[o + c] + a.cx[o + c];
        const f32x4 dz = d * ww[k] * acf_step4(z);
        a.da[o + c] = dz;
        a.dprof[o + c] = al * dd[k];
        su[k] += dz;
        sw[k] += d * acf_relu4(z);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < CH; ++k) {
    const int c = threadIdx.x + k * 256;
    if (c < a.ev) {
      a.duw[(int64_t)b * a.ev + c] = dd[k] + su[k];
      a.dwp[(int64_t)b * a.ev + c] = sw[k];
    }
  }
}

}  // namespace pxr

using namespace pxr;

#define ACF_LAUNCH_CH(kernel, grid, st, args)                                                   \
  do {                                                                                          \
    const int ch_ = ((args).ev + 255) / 256;                                                    \
    if (ch_ <= 1) hipLaunchKernelGGL(kernel<1>, grid, dim3(256), 0, st, args);                  \
    else if (ch_ <= 2) hipLaunchKernelGGL(kernel<2>, grid, dim3(256), 0, st, args);             \
    else hipLaunchKernelGGL(kernel<4>, grid, dim3(256), 0, st, args);                           \
  } while (0)

static inline bool acf_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int acf_region_shape_ok(const char* who, int B, int P, int H, int E) {
  PXR_REQUIRE(B > 0 && P > 0 && (int64_t)B * P < (1ll << 31), "%s: need B > 0, P > 0 and B P < 2^31 (B=%d, P=%d)", who, B, P);
  PXR_REQUIRE(H > 0 && H <= ACF_MAX_N, "%s: need 0 < H <= %d regions (H=%d)", who, ACF_MAX_N, H);
  PXR_REQUIRE(E > 0 && E % 4 == 0 && E <= 4096, "%s: need E %% 4 == 0 and 0 < E <= 4096 (E=%d)", who, E);
  return PXR_OK;
}

extern "C" int pxr_acf_region_fwd_f32(const float* x, const float* xt, const float* ut, const float* w, const int64_t* profile,
                                      int B, int P, int H, int E, float* beta, float* pooled, void* stream) {
  PXR_REQUIRE(x && xt && ut && w && profile && beta && pooled, "pxr_acf_region_fwd_f32: null pointer");
  if (int rc = acf_region_shape_ok("pxr_acf_region_fwd_f32", B, P, H, E)) return rc;
  PXR_REQUIRE(acf_aligned(x) && acf_aligned(xt) && acf_aligned(ut) && acf_aligned(w) && acf_aligned(pooled),
              "pxr_acf_region_fwd_f32: operands must be 16-byte aligned");
  AcfRegionArgs a{};
  a.x = (const f32x4*)x; a.xt = (const f32x4*)xt; a.ut = (const f32x4*)ut; a.w = (const f32x4*)w; a.profile = profile;
  a.beta = beta; a.pooled = (f32x4*)pooled; a.R = B * P; a.P = P; a.H = H; a.ev = E / 4;
  hipStream_t st = (hipStream_t)stream;
  ACF_LAUNCH_CH(acf_region_fwd_kernel, dim3((unsigned)a.R), st, a);
  return pxr_check_launch("pxr_acf_region_fwd_f32");
}

extern "C" int pxr_acf_region_bwd_f32(const float* dpooled, const float* x, const float* xt, const float* ut, const float* w,
                                      const int64_t* profile, const float* beta, int B, int P, int H, int E, float* dxt,
                                      float* dut, float* dw_part, float* ws, void* stream) {
  PXR_REQUIRE(dpooled && x && xt && ut && w && profile && beta && dxt && dut && dw_part && ws,
              "pxr_acf_region_bwd_f32: null pointer");
  if (int rc = acf_region_shape_ok("pxr_acf_region_bwd_f32", B, P, H, E)) return rc;
  PXR_REQUIRE(acf_aligned(dpooled) && acf_aligned(x) && acf_aligned(xt) && acf_aligned(ut) && acf_aligned(w) && acf_aligned(dxt) &&
                  acf_aligned(dut) && acf_aligned(dw_part) && acf_aligned(ws),
              "pxr_acf_region_bwd_f32: operands must be 16-byte aligned");
  PXR_REQUIRE(dxt != xt && dxt != x, "pxr_acf_region_bwd_f32: dxt must not alias x or xt");
  AcfRegionArgs a{};
  a.x = (const f32x4*)x; a.xt = (const f32x4*)xt; a.ut = (const f32x4*)ut; a.w = (const f32x4*)w; a.profile = profile;
  a.beta = (float*)beta; a.dpooled = (const f32x4*)dpooled; a.dxt = (f32x4*)dxt; a.dutp = (f32x4*)ws; a.dwp = (f32x4*)dw_part;
  a.R = B * P; a.P = P; a.H = H; a.ev = E / 4;
  hipStream_t st = (hipStream_t)stream;
  ACF_LAUNCH_CH(acf_region_bwd_kernel, dim3((unsigned)a.R), st, a);
  int rc = pxr_check_launch("pxr_acf_region_bwd_f32");
  if (rc) return rc;
  const int64_t n = (int64_t)B * a.ev;
  hipLaunchKernelGGL(acf_group_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const f32x4*)ws, (f32x4*)dut, B, P,
                     a.ev);
  return pxr_check_launch("pxr_acf_region_bwd_f32 (group sum)");
}

extern "C" int pxr_acf_region_dx_f32(float* dx, const float* x, const float* beta, const float* dpooled, int64_t R, int H, int E,
                                     void* stream) {
  PXR_REQUIRE(dx && x && beta && dpooled, "pxr_acf_region_dx_f32: null pointer");
  PXR_REQUIRE(R > 0 && H > 0 && R * H < (1ll << 31), "pxr_acf_region_dx_f32: need 0 < R H < 2^31");
  PXR_REQUIRE(E > 0 && E % 4 == 0 && E <= 4096, "pxr_acf_region_dx_f32: need E %% 4 == 0 and 0 < E <= 4096 (E=%d)", E);
  PXR_REQUIRE(acf_aligned(dx) && acf_aligned(x) && acf_aligned(dpooled), "pxr_acf_region_dx_f32: operands must be 16-byte aligned");
  const int64_t total = R * H * (E / 4);
  int64_t blocks = (total + 255) / 256;
  if (blocks > 256 * 256) blocks = 256 * 256;
  hipLaunchKernelGGL(acf_region_dx_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (f32x4*)dx, (const f32x4*)x, beta,
                     (const f32x4*)dpooled, R * H, H, E / 4);
  return pxr_check_launch("pxr_acf_region_dx_f32");
}

static int acf_item_shape_ok(const char* who, int B, int P, int E) {
  PXR_REQUIRE(B > 0 && P > 0 && P <= ACF_MAX_N && (int64_t)B * P < (1ll << 31), "%s: need B > 0 and 0 < P <= %d (B=%d, P=%d)", who,
              ACF_MAX_N, B, P);
  PXR_REQUIRE(E > 0 && E % 4 == 0 && E <= 4096, "%s: need E %% 4 == 0 and 0 < E <= 4096 (E=%d)", who, E);
  return PXR_OK;
}

extern "C" int pxr_acf_item_fwd_f32(const float* uw, const float* pq, const float* cx, const float* prof, const float* w,
                                    const int64_t* profile, int B, int P, int E, float* alpha, float* user, void* stream) {
  PXR_REQUIRE(uw && pq && cx && prof && w && profile && alpha && user, "pxr_acf_item_fwd_f32: null pointer");
  if (int rc = acf_item_shape_ok("pxr_acf_item_fwd_f32", B, P, E)) return rc;
  PXR_REQUIRE(acf_aligned(uw) && acf_aligned(pq) && acf_aligned(cx) && acf_aligned(prof) && acf_aligned(w) && acf_aligned(user),
              "pxr_acf_item_fwd_f32: operands must be 16-byte aligned");
  AcfItemArgs a{};
  a.uw = (const f32x4*)uw; a.pq = (const f32x4*)pq; a.cx = (const f32x4*)cx; a.prof = (const f32x4*)prof; a.w = (const f32x4*)w;
  a.profile = profile; a.alpha = alpha; a.user = (f32x4*)user; a.B = B; a.P = P; a.ev = E / 4;
  hipStream_t st = (hipStream_t)stream;
  ACF_LAUNCH_CH(acf_item_fwd_kernel, dim3((unsigned)B), st, a);
  return pxr_check_launch("pxr_acf_item_fwd_f32");
}

extern "C" int pxr_acf_item_bwd_f32(const float* duser, const float* uw, const float* pq, const float* cx, const float* prof,
                                    const float* w, const float* alpha, int B, int P, int E, float* da, float* dprof, float* duw,
                                    float* dw_part, void* stream) {
  PXR_REQUIRE(duser && uw && pq && cx && prof && w && alpha && da && dprof && duw && dw_part, "pxr_acf_item_bwd_f32: null pointer");
  if (int rc = acf_item_shape_ok("pxr_acf_item_bwd_f32", B, P, E)) return rc;
  PXR_REQUIRE(acf_aligned(duser) && acf_aligned(uw) && acf_aligned(pq) && acf_aligned(cx) && acf_aligned(prof) && acf_aligned(w) &&
                  acf_aligned(da) && acf_aligned(dprof) && acf_aligned(duw) && acf_aligned(dw_part),
              "pxr_acf_item_bwd_f32: operands must be 16-byte aligned");
  PXR_REQUIRE(da != pq && da != cx && dprof != prof && duw != duser && duw != uw,
              "pxr_acf_item_bwd_f32: outputs must not alias inputs");
  AcfItemArgs a{};
  a.duser = (const f32x4*)duser; a.uw = (const f32x4*)uw; a.pq = (const f32x4*)pq; a.cx = (const f32x4*)cx; a.prof = (const f32x4*)prof;
  a.w = (const f32x4*)w; a.alpha = (float*)alpha; a.da = (f32x4*)da; a.dprof = (f32x4*)dprof; a.duw = (f32x4*)duw; a.dwp = (f32x4*)dw_part;
  a.B = B; a.P = P; a.ev = E / 4;
  hipStream_t st = (hipStream_t)stream;
  ACF_LAUNCH_CH(acf_item_bwd_kernel, dim3((unsigned)B), st, a);
  return pxr_check_launch("pxr_acf_item_bwd_f32");
}
