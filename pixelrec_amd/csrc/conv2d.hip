// conv2d.hip -- the index kernels of the CNN-F image encoder (reference code/REC/model/PixelNet/dvbpr.py:113-137: five Conv2d +
// ReLU, three of them under MaxPool2d(2)).  A convolution here is EXPLICIT im2col over a bounded chunk of images with the library
// GEMMs doing the product (y = col W^T + b with the ReLU epilogue, dW = dY^T col, dcol = dY W): this file holds what surrounds
// those GEMMs -- im2col, its gather-form inverse col2im, the 2x2 max-pool and the pool's backward fused with the ReLU mask.
//
// Geometry: padding 0, dilation 1, any kernel kh x kw and stride sh x sw with Ho = (H - kh) / sh + 1, Wo = (W - kw) / sw + 1 (floor).
// The pool is 2 x 2, stride 2, floor mode: Hp = H / 2, Wp = W / 2, a trailing odd row / column is dropped.
// Layouts: an activation is addressed through four element strides (n, c, h, w), so the image (NCHW) and the GEMM outputs (NHWC: a
// [n Ho Wo, Cout] GEMM result IS the next layer's input) go through the same kernels; the column order of im2col is (cin, kh, kw),
// so weight.view(Cout, Cin kh kw) is the GEMM's B operand as it stands.  Every offset is 64-bit.  fp32 throughout, no atomics: each
// output element is written once by one thread, and every sum has one fixed order.
#include "pxr_common.h"

namespace pxr {

struct Conv2dGeom {
  int64_t n;
  int C, H, W, kh, kw, sh, sw, Ho, Wo;
};

// element strides of an activation
struct Act4 {
  int64_t sn, sc, sh, sw;
};

// col[row, k] = x[img, c, ho sh + i, wo sw + j] for row = (img, ho, wo), k = (c, i, j); k in [K, ldk) gets +0.0.  One thread per
// float4 of a row: four gathered loads, one 16-byte store.
__global__ void __launch_bounds__(256) conv2d_im2col_kernel(const float* __restrict__ x, Act4 xs, Conv2dGeom g, int K, int ldk4,
                                                             int64_t total4, f32x4* __restrict__ col) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total4) return;
  const int64_t row = t / ldk4;
  const int k0 = (int)(t - row * ldk4) * 4;
  const int64_t img = row / ((int64_t)g.Ho * g.Wo);
  const int r = (int)(row - img * ((int64_t)g.Ho * g.Wo));
  const int ho = r / g.Wo, wo = r - ho * g.Wo;
  const float* base = x + img * xs.sn + (int64_t)(ho * g.sh) * xs.sh + (int64_t)(wo * g.sw) * xs.sw;
  const int kk = g.kh * g.kw;
  float v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = k0 + q;
    if (k < K) {
      const int c = k / kk, ij = k - c * kk;
      const int i = ij / g.kw, j = ij - i * g.kw;
      v[q] = base[c * xs.sc + i * xs.sh + j * xs.sw];
    } else {
      v[q] = 0.f;
    }
  }
  col[t] = f32x4{v[0], v[1], v[2], v[3]};
}

// The data gradient in gather form: dx[img, c, h, w] = sum over the windows that read the element, kh outer, kw inner:
//   for i in [0, kh), j in [0, kw): ho = (h - i) / sh, wo = (w - j) / sw when both divide and lie in the output -> dcol[(img, ho,
//   wo), (c, i, j)].  An element no window covers (a stride remainder) gets +0.0.  VEC: dx is NHWC-dense in c (sc == 1, C % 4 == 0)
// and a thread owns four channels of one pixel -- four strided loads per window, one 16-byte store; else one element per thread.
template <bool VEC>
__global__ void __launch_bounds__(256) conv2d_col2im_kernel(const float* __restrict__ dcol, int64_t ldk, Conv2dGeom g, Act4 ds,
                                                             int64_t total, float* __restrict__ dx) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  constexpr int CV = VEC ? 4 : 1;
  const int cg = g.C / CV;
  // t = ((img H + h) W + w) cg + c / CV
  const int c = (int)(t % cg) * CV;
  const int64_t p = t / cg;
  const int w = (int)(p % g.W);
  const int64_t q2 = p / g.W;
  const int h = (int)(q2 % g.H);
  const int64_t img = q2 / g.H;
  const int kk = g.kh * g.kw;
  float s[CV];
#pragma unroll
  for (int q = 0; q < CV; ++q) s[q] = 0.f;
  for (int i = 0; i < g.kh; ++i) {
    const int hh = h - i;
    if (hh < 0) break;
    if (hh % g.sh) continue;
    const int ho = hh / g.sh;
    if (ho >= g.Ho) continue;
    for (int j = 0; j < g.kw; ++j) {
      const int ww = w - j;
      if (ww < 0) break;
      if (ww % g.sw) continue;
      const int wo = ww / g.sw;
      if (wo >= g.Wo) continue;
      const float* src = dcol + ((img * g.Ho + ho) * g.Wo + wo) * ldk + (int64_t)c * kk + i * g.kw + j;
#pragma unroll
      for (int q = 0; q < CV; ++q) s[q] += src[q * kk];
    }
  }
  float* dst = dx + img * ds.sn + (int64_t)h * ds.sh + (int64_t)w * ds.sw + (int64_t)c * ds.sc;
  if (VEC) {
    *reinterpret_cast<f32x4*>(dst) = f32x4{s[0], s[CV > 1 ? 1 : 0], s[CV > 1 ? 2 : 0], s[CV > 1 ? 3 : 0]};
  } else {
    dst[0] = s[0];
  }
}

// winner of the 2 x 2 window in row-major order (0 .. 3): the FIRST of equal values, torch's rule (a later element replaces the
// maximum only when it is strictly greater)
__device__ __forceinline__ int pool_argmax(float a, float b, float c, float d, float& m) {
  int k = 0;
  m = a;
  if (b > m) { m = b; k = 1; }
  if (c > m) { m = c; k = 2; }
  if (d > m) { m = d; k = 3; }
  return k;
}

// p[img, c, hp, wp] = max of y[img, c, 2hp .. 2hp + 1, 2wp .. 2wp + 1].  VEC: both sides dense in c, four channels per thread.
template <bool VEC>
__global__ void __launch_bounds__(256) conv2d_pool_fwd_kernel(const float* __restrict__ y, Act4 ys, int C, int Hp, int Wp, Act4 ps,
                                                               int64_t total, float* __restrict__ p) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  constexpr int CV = VEC ? 4 : 1;
  const int cg = C / CV;
  const int c = (int)(t % cg) * CV;
  const int64_t r = t / cg;
  const int wp = (int)(r % Wp);
  const int64_t r2 = r / Wp;
  const int hp = (int)(r2 % Hp);
  const int64_t img = r2 / Hp;
  const float* s00 = y + img * ys.sn + (int64_t)(2 * hp) * ys.sh + (int64_t)(2 * wp) * ys.sw + (int64_t)c * ys.sc;
  float* dst = p + img * ps.sn + (int64_t)hp * ps.sh + (int64_t)wp * ps.sw + (int64_t)c * ps.sc;
  if (VEC) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(s00), b = *reinterpret_cast<const f32x4*>(s00 + ys.sw);
    const f32x4 cc = *reinterpret_cast<const f32x4*>(s00 + ys.sh), d = *reinterpret_cast<const f32x4*>(s00 + ys.sh + ys.sw);
    float m0, m1, m2, m3;
    pool_argmax(a.x, b.x, cc.x, d.x, m0);
    pool_argmax(a.y, b.y, cc.y, d.y, m1);
    pool_argmax(a.z, b.z, cc.z, d.z, m2);
    pool_argmax(a.w, b.w, cc.w, d.w, m3);
    *reinterpret_cast<f32x4*>(dst) = f32x4{m0, m1, m2, m3};
  } else {
    float m;
    pool_argmax(s00[0], s00[ys.sw], s00[ys.sh], s00[ys.sh + ys.sw], m);
    dst[0] = m;
  }
}

// dy[pix] = dp[window of pix] where pix is its window's winner and y[pix] > 0 (the ReLU in front of the pool), else +0.0; the rows
// and columns that floor mode drops get +0.0.  y is the ReLU'd conv output the forward pooled.  One thread per element of dy (VEC:
// four channels), so every element is written exactly once.
template <bool VEC>
__global__ void __launch_bounds__(256) conv2d_pool_bwd_kernel(const float* __restrict__ y, Act4 ys, const float* __restrict__ dp,
                                                               Act4 ps, int C, int H, int W, int Hp, int Wp, int64_t total,
                                                               float* __restrict__ dy) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  constexpr int CV = VEC ? 4 : 1;
  const int cg = C / CV;
  const int c = (int)(t % cg) * CV;
  const int64_t r = t / cg;
  const int w = (int)(r % W);
  const int64_t r2 = r / W;
  const int h = (int)(r2 % H);
  const int64_t img = r2 / H;
  const int hp = h >> 1, wp = w >> 1;
  float* dst = dy + img * ys.sn + (int64_t)h * ys.sh + (int64_t)w * ys.sw + (int64_t)c * ys.sc;   // dy has y's layout
  float out[CV];
#pragma unroll
  for (int q = 0; q < CV; ++q) out[q] = 0.f;
  if (hp < Hp && wp < Wp) {
    const float* s00 = y + img * ys.sn + (int64_t)(2 * hp) * ys.sh + (int64_t)(2 * wp) * ys.sw + (int64_t)c * ys.sc;
    const float* g = dp + img * ps.sn + (int64_t)hp * ps.sh + (int64_t)wp * ps.sw + (int64_t)c * ps.sc;
    const int me = (h & 1) * 2 + (w & 1);
#pragma unroll
    for (int q = 0; q < CV; ++q) {
      const float* s = s00 + q * ys.sc;
      float m;
      const int k = pool_argmax(s[0], s[ys.sw], s[ys.sh], s[ys.sh + ys.sw], m);
      if (k == me && m > 0.f) out[q] = g[q * ps.sc];
    }
  }
  if (VEC) {
    *reinterpret_cast<f32x4*>(dst) = f32x4{out[0], out[CV > 1 ? 1 : 0], out[CV > 1 ? 2 : 0], out[CV > 1 ? 3 : 0]};
  } else {
    dst[0] = out[0];
  }
}

static inline bool blocks_ok(int64_t total) { return total > 0 && (total + 255) / 256 < (1ll << 31); }

// the geometry every entry checks before it launches
static inline const char* conv_geom_error(int64_t n, int C, int H, int W, int kh, int kw, int sh, int sw) {
  if (n <= 0 || C <= 0 || H <= 0 || W <= 0) return "empty input";
  if (kh <= 0 || kw <= 0) return "empty kernel";
  if (sh <= 0 || sw <= 0) return "stride must be positive";
  if (kh > H || kw > W) return "kernel larger than the input";
  if ((int64_t)C * kh * kw >= (1ll << 31)) return "C kh kw too large";
  return nullptr;
}

}  // namespace pxr

using namespace pxr;

#define CONV_GEOM(name)                                                                                                        \
  {                                                                                                                            \
    const char* why = conv_geom_error(n, C, H, W, kh, kw, sh, sw);                                                             \
    PXR_REQUIRE(!why, name ": %s (n=%lld C=%d H=%d W=%d kernel %dx%d stride %dx%d)", why, (long long)n, C, H, W, kh, kw, sh, sw); \
  }

extern "C" int pxr_conv2d_im2col_f32(const float* x, int64_t x_sn, int64_t x_sc, int64_t x_sh, int64_t x_sw, int64_t n, int C, int H,
                                     int W, int kh, int kw, int sh, int sw, float* col, int64_t ldk, void* stream) {
  PXR_REQUIRE(x && col, "pxr_conv2d_im2col_f32: null pointer");
  CONV_GEOM("pxr_conv2d_im2col_f32");
  const int K = C * kh * kw;
  PXR_REQUIRE(ldk % 4 == 0 && ldk >= K && ldk < K + 4, "pxr_conv2d_im2col_f32: ldk must be K = %d rounded up to a multiple of 4 (ldk=%lld)",
              K, (long long)ldk);
  PXR_REQUIRE(((uintptr_t)col & 15) == 0, "pxr_conv2d_im2col_f32: col must be 16-byte aligned");
  PXR_REQUIRE(x_sn > 0 && x_sc > 0 && x_sh > 0 && x_sw > 0, "pxr_conv2d_im2col_f32: strides must be positive");
  Conv2dGeom g{n, C, H, W, kh, kw, sh, sw, (H - kh) / sh + 1, (W - kw) / sw + 1};
  const int64_t total4 = n * g.Ho * g.Wo * (ldk / 4);
  PXR_REQUIRE(blocks_ok(total4), "pxr_conv2d_im2col_f32: too many columns for one launch (cut the chunk)");
  hipLaunchKernelGGL(conv2d_im2col_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                     Act4{x_sn, x_sc, x_sh, x_sw}, g, K, (int)(ldk / 4), total4, (f32x4*)col);
  return pxr_check_launch("pxr_conv2d_im2col_f32");
}

extern "C" int pxr_conv2d_col2im_f32(const float* dcol, int64_t ldk, int64_t n, int C, int H, int W, int kh, int kw, int sh, int sw,
                                     float* dx, int64_t d_sn, int64_t d_sc, int64_t d_sh, int64_t d_sw, void* stream) {
  PXR_REQUIRE(dcol && dx, "pxr_conv2d_col2im_f32: null pointer");
  CONV_GEOM("pxr_conv2d_col2im_f32");
  const int K = C * kh * kw;
  PXR_REQUIRE(ldk % 4 == 0 && ldk >= K && ldk < K + 4, "pxr_conv2d_col2im_f32: ldk must be K = %d rounded up to a multiple of 4 (ldk=%lld)",
              K, (long long)ldk);
  PXR_REQUIRE(d_sn > 0 && d_sc > 0 && d_sh > 0 && d_sw > 0, "pxr_conv2d_col2im_f32: strides must be positive");
  Conv2dGeom g{n, C, H, W, kh, kw, sh, sw, (H - kh) / sh + 1, (W - kw) / sw + 1};
  const bool vec = d_sc == 1 && C % 4 == 0 && d_sn % 4 == 0 && d_sh % 4 == 0 && d_sw % 4 == 0 && ((uintptr_t)dx & 15) == 0;
  const int64_t total = n * H * W * (C / (vec ? 4 : 1));
  PXR_REQUIRE(blocks_ok(total), "pxr_conv2d_col2im_f32: too many elements for one launch (cut the chunk)");
  const dim3 grid((unsigned)((total + 255) / 256));
  if (vec)
    hipLaunchKernelGGL(conv2d_col2im_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, dcol, ldk, g,
                       Act4{d_sn, d_sc, d_sh, d_sw}, total, dx);
  else
    hipLaunchKernelGGL(conv2d_col2im_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, dcol, ldk, g,
                       Act4{d_sn, d_sc, d_sh, d_sw}, total, dx);
  return pxr_check_launch("pxr_conv2d_col2im_f32");
}

static inline bool act_vec_ok(const void* p, int C, int64_t sn, int64_t sc, int64_t sh, int64_t sw) {
  return sc == 1 && C % 4 == 0 && sn % 4 == 0 && sh % 4 == 0 && sw % 4 == 0 && ((uintptr_t)p & 15) == 0;
}

extern "C" int pxr_maxpool2x2_fwd_f32(const float* y, int64_t y_sn, int64_t y_sc, int64_t y_sh, int64_t y_sw, int64_t n, int C, int H,
                                      int W, float* p, int64_t p_sn, int64_t p_sc, int64_t p_sh, int64_t p_sw, void* stream) {
  PXR_REQUIRE(n > 0 && C > 0 && H >= 2 && W >= 2, "pxr_maxpool2x2_fwd_f32: need n, C > 0 and H, W >= 2 (n=%lld C=%d H=%d W=%d)",
              (long long)n, C, H, W);
  PXR_REQUIRE(y && p, "pxr_maxpool2x2_fwd_f32: null pointer");
  PXR_REQUIRE(y_sn > 0 && y_sc > 0 && y_sh > 0 && y_sw > 0 && p_sn > 0 && p_sc > 0 && p_sh > 0 && p_sw > 0,
              "pxr_maxpool2x2_fwd_f32: strides must be positive");
  const int Hp = H / 2, Wp = W / 2;
  const bool vec = act_vec_ok(y, C, y_sn, y_sc, y_sh, y_sw) && act_vec_ok(p, C, p_sn, p_sc, p_sh, p_sw);
  const int64_t total = n * Hp * Wp * (C / (vec ? 4 : 1));
  PXR_REQUIRE(blocks_ok(total), "pxr_maxpool2x2_fwd_f32: too many elements for one launch");
  const dim3 grid((unsigned)((total + 255) / 256));
  const Act4 ys{y_sn, y_sc, y_sh, y_sw}, ps{p_sn, p_sc, p_sh, p_sw};
  if (vec) hipLaunchKernelGGL(conv2d_pool_fwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, y, ys, C, Hp, Wp, ps, total, p);
  else hipLaunchKernelGGL(conv2d_pool_fwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, y, ys, C, Hp, Wp, ps, total, p);
  return pxr_check_launch("pxr_maxpool2x2_fwd_f32");
}

extern "C" int pxr_maxpool2x2_relu_bwd_f32(const float* y, int64_t y_sn, int64_t y_sc, int64_t y_sh, int64_t y_sw, const float* dp,
                                           int64_t p_sn, int64_t p_sc, int64_t p_sh, int64_t p_sw, int64_t n, int C, int H, int W,
                                           float* dy, void* stream) {
  PXR_REQUIRE(y && dp && dy, "pxr_maxpool2x2_relu_bwd_f32: null pointer");
  PXR_REQUIRE(n > 0 && C > 0 && H >= 2 && W >= 2, "pxr_maxpool2x2_relu_bwd_f32: need n, C > 0 and H, W >= 2 (n=%lld C=%d H=%d W=%d)",
              (long long)n, C, H, W);
  PXR_REQUIRE(y_sn > 0 && y_sc > 0 && y_sh > 0 && y_sw > 0 && p_sn > 0 && p_sc > 0 && p_sh > 0 && p_sw > 0,
              "pxr_maxpool2x2_relu_bwd_f32: strides must be positive");
  const bool vec = act_vec_ok(y, C, y_sn, y_sc, y_sh, y_sw) && ((uintptr_t)dy & 15) == 0;
  const int64_t total = n * H * W * (C / (vec ? 4 : 1));
  PXR_REQUIRE(blocks_ok(total), "pxr_maxpool2x2_relu_bwd_f32: too many elements for one launch");
  const dim3 grid((unsigned)((total + 255) / 256));
  const Act4 ys{y_sn, y_sc, y_sh, y_sw}, ps{p_sn, p_sc, p_sh, p_sw};
  if (vec)
    hipLaunchKernelGGL(conv2d_pool_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, y, ys, dp, ps, C, H, W, H / 2, W / 2, total, dy);
  else
    hipLaunchKernelGGL(conv2d_pool_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, y, ys, dp, ps, C, H, W, H / 2, W / 2, total, dy);
  return pxr_check_launch("pxr_maxpool2x2_relu_bwd_f32");
}
