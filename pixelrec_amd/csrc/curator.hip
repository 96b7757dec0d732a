// curator.hip -- CuratorNet (reference code/REC/model/ViNet/curatornet.py): the profile pooling between the "common" tower and the
// profile tower, forward and backward.
//
// Forward (curatornet.py:77-79, predict :96-99): cat[b, :] = [max over l of h[b, l, :] | mean over l of h[b, l, :]] over ALL L
// positions, padded ones included (AdaptiveMaxPool2d / AdaptiveAvgPool2d((1, E)) on [B, L, E]); the mean divides by L.  The max
// keeps the FIRST position among equal values (torch's rule; padded positions are the same row and tie exactly).  Rows are read in
// place from the tower's output (training) or gathered from the item matrix by id (predict's item_feature[user]).
//
// Backward: ONE launch writes the gradient of the second common Linear's pre-activation for every row of the step's
// [B L profile rows | 2B positive / negative rows] block -- mean and max paths joined, SELU derivative applied.  Every output
// element is written by exactly one thread: no read-modify-write, no atomics, bit-identical from run to run.
//
// Pair head (curatornet.py:86-88): the 1e-8 sits INSIDE the log there, as in vbpr.py and unlike mf.py, so a badly ranked pair
// saturates at -log(1e-8) and its gradient fades; the backward is MF's (pxr_mf_pair_bwd_f32 needs coef alone).
//
// The pooling kernels are bandwidth-bound: one thread per four columns, 16-byte accesses, a loop over L.
#include "pair_head.cuh"

namespace pxr {

struct CuratorPoolArgs {
  const f32x4* h;              // [B L, ev] (ids == NULL) or [n_items, ev]
  const int64_t* ids;          // [B, L] or NULL
  int64_t n_items;
  int B, L, ev;                // ev = E / 4
  f32x4* cat;                  // [B, 2 ev]
  uint32_t* argmax;            // [B, ev] (four uint8 positions per word) or NULL
};

__global__ void __launch_bounds__(256) curator_pool_kernel(CuratorPoolArgs a, int32_t* status) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)a.B * a.ev) return;
  const int b = (int)(t / a.ev), c = (int)(t % a.ev);
  f32x4 mx = {0.f, 0.f, 0.f, 0.f}, sum = {0.f, 0.f, 0.f, 0.f};
  uint32_t ax = 0, ay = 0, az = 0, aw = 0;
  for (int l = 0; l < a.L; ++l) {
    int64_t row = (int64_t)b * a.L + l;
    if (a.ids) row = checked_id(a.ids[row], a.n_items, status, true);
    const f32x4 v = a.h[row * a.ev + c];
    sum += v;
    if (l == 0) {
      mx = v;
    } else {       // strictly greater: the first of equal values stays
      if (v.x > mx.x) { mx.x = v.x; ax = l; }
      if (v.y > mx.y) { mx.y = v.y; ay = l; }
      if (v.z > mx.z) { mx.z = v.z; az = l; }
      if (v.w > mx.w) { mx.w = v.w; aw = l; }
    }
  }
  a.cat[(int64_t)b * 2 * a.ev + c] = mx;
  a.cat[(int64_t)b * 2 * a.ev + a.ev + c] = sum / (float)a.L;       // by L, not by the number of real items
  if (a.argmax) a.argmax[t] = ax | (ay << 8) | (az << 16) | (aw << 24);
}

struct CuratorPoolBwdArgs {
  const f32x4* dcat;           // [B, 2 ev]: gradient of [max | mean]
  const uint32_t* argmax;      // [B, ev]
  const f32x4* di;             // [2B, ev]: the pair head's gradient onto the positive / negative rows
  const f32x4* dact;           // [B (L + 2), ev]: selu' of the second common Linear, saved by its forward
  int B, L, ev;
  f32x4* dpre;                 // [B (L + 2), ev]
};

__global__ void __launch_bounds__(256) curator_pool_bwd_kernel(CuratorPoolBwdArgs a) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n_prof = (int64_t)a.B * a.L;
  if (t >= (n_prof + 2 * (int64_t)a.B) * a.ev) return;
  const int64_t row = t / a.ev;
  const int c = (int)(t % a.ev);
  f32x4 g;
  if (row < n_prof) {
    const int b = (int)(row / a.L);
    const uint32_t l = (uint32_t)(row % a.L);
    const f32x4 dmax = a.dcat[(int64_t)b * 2 * a.ev + c];
    const uint32_t am = a.argmax[(int64_t)b * a.ev + c];
    g = a.dcat[(int64_t)b * 2 * a.ev + a.ev + c] / (float)a.L;
    if ((am & 255u) == l) g.x += dmax.x;
    if (((am >> 8) & 255u) == l) g.y += dmax.y;
    if (((am >> 16) & 255u) == l) g.z += dmax.z;
    if ((am >> 24) == l) g.w += dmax.w;
  } else {
    g = a.di[(row - n_prof) * a.ev + c];
  }
  a.dpre[t] = g * a.dact[t];
}

// out = a * b over n / 4 vectors (the head's user gradient through selu_pu3's saved derivative: no GEMM stands in front of it)
__global__ void __launch_bounds__(256) curator_mul_kernel(const f32x4* __restrict__ x, const f32x4* __restrict__ y, f32x4* __restrict__ out,
                                                           int64_t nv) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < nv) out[t] = x[t] * y[t];
}

// x_b = <u_b, i+_b> - <u_b, i-_b> on the towers' outputs (u [B, hv], it [2B, hv] = positive, negative per sample) into the tail
// with the 1e-8 inside the log.  One wave per b.
__global__ void __launch_bounds__(256) curator_pair_fwd_kernel(const f32x4* __restrict__ u, const f32x4* __restrict__ it, int hv, int B,
                                                                float* __restrict__ coef, float* __restrict__ lossrow) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  float sp, sn;
  pair_dots(u + (int64_t)b * hv, it + 2 * (int64_t)b * hv, it + (2 * (int64_t)b + 1) * hv, hv, lane, sp, sn);
  if (lane == 0) bpr_tail_log_inside(sp - sn, B, lossrow[b], coef[b]);
}

}  // namespace pxr

using namespace pxr;

extern "C" int pxr_curator_pair_fwd_f32(const float* ufeat, const float* ifeat, int H, int B, float* coef, float* lossrow,
                                        float* loss, void* stream) {
  PXR_REQUIRE(ufeat && ifeat && coef && lossrow && loss, "pxr_curator_pair_fwd_f32: null pointer");
  PXR_REQUIRE(H > 0 && H % 4 == 0 && H <= 4096, "pxr_curator_pair_fwd_f32: need H %% 4 == 0 and 0 < H <= 4096 (H=%d)", H);
  PXR_REQUIRE(B > 0 && B <= (1 << 28), "pxr_curator_pair_fwd_f32: bad batch size %d", B);
  PXR_REQUIRE((((uintptr_t)ufeat | (uintptr_t)ifeat) & 15) == 0, "pxr_curator_pair_fwd_f32: features must be 16-byte aligned");
  hipLaunchKernelGGL(curator_pair_fwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)ufeat,
                     (const f32x4*)ifeat, H / 4, B, coef, lossrow);
  const int rc = pxr_check_launch("pxr_curator_pair_fwd_f32");
  if (rc) return rc;
  return pxr_bpr_loss_reduce(lossrow, B, 1, loss, stream);        // loss = (1/B) sum_b lossrow[b], fixed order
}

extern "C" int pxr_mul_f32(const float* a, const float* b, float* out, int64_t n, void* stream) {
  PXR_REQUIRE(a && b && out && n > 0 && n % 4 == 0 && n <= (1ll << 38), "pxr_mul_f32: bad args (n must be a positive multiple of 4)");
  PXR_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)out) & 15) == 0, "pxr_mul_f32: operands must be 16-byte aligned");
  hipLaunchKernelGGL(curator_mul_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)a,
                     (const f32x4*)b, (f32x4*)out, n / 4);
  return pxr_check_launch("pxr_mul_f32");
}

extern "C" int pxr_curator_pool_f32(const float* h, const int64_t* ids, int64_t n_items, int B, int L, int E, float* cat,
                                    uint8_t* argmax, void* stream) {
  PXR_REQUIRE(h && cat, "pxr_curator_pool_f32: null pointer");
  PXR_REQUIRE(E > 0 && E % 4 == 0 && E <= 4096, "pxr_curator_pool_f32: need E %% 4 == 0 and 0 < E <= 4096 (E=%d)", E);
  PXR_REQUIRE(L >= 1 && L <= 255, "pxr_curator_pool_f32: need 1 <= L <= 255 (the argmax is stored in a byte), got L=%d", L);
  PXR_REQUIRE(B > 0 && (int64_t)B * L <= (1ll << 28), "pxr_curator_pool_f32: bad batch size %d", B);
  PXR_REQUIRE(!ids || (n_items > 0 && n_items < (1ll << 40)), "pxr_curator_pool_f32: bad item count %lld", (long long)n_items);
  PXR_REQUIRE((((uintptr_t)h | (uintptr_t)cat) & 15) == 0 && ((uintptr_t)argmax & 3) == 0,
              "pxr_curator_pool_f32: operands must be 16-byte aligned (argmax: 4-byte)");
  CuratorPoolArgs a{(const f32x4*)h, ids, n_items, B, L, E / 4, (f32x4*)cat, (uint32_t*)argmax};
  const int64_t n = (int64_t)B * a.ev;
  hipLaunchKernelGGL(curator_pool_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a,
                     ids ? pxr_status_word() : nullptr);
  return pxr_check_launch("pxr_curator_pool_f32");
}

extern "C" int pxr_curator_pool_bwd_f32(const float* dcat, const uint8_t* argmax, const float* di, const float* dact, int B, int L,
                                        int E, float* dpre, void* stream) {
  PXR_REQUIRE(dcat && argmax && di && dact && dpre, "pxr_curator_pool_bwd_f32: null pointer");
  PXR_REQUIRE(E > 0 && E % 4 == 0 && E <= 4096, "pxr_curator_pool_bwd_f32: need E %% 4 == 0 and 0 < E <= 4096 (E=%d)", E);
  PXR_REQUIRE(L >= 1 && L <= 255, "pxr_curator_pool_bwd_f32: need 1 <= L <= 255, got L=%d", L);
  PXR_REQUIRE(B > 0 && (int64_t)B * (L + 2) <= (1ll << 28), "pxr_curator_pool_bwd_f32: bad batch size %d", B);
  PXR_REQUIRE((((uintptr_t)dcat | (uintptr_t)di | (uintptr_t)dact | (uintptr_t)dpre) & 15) == 0 && ((uintptr_t)argmax & 3) == 0,
              "pxr_curator_pool_bwd_f32: operands must be 16-byte aligned (argmax: 4-byte)");
  CuratorPoolBwdArgs a{(const f32x4*)dcat, (const uint32_t*)argmax, (const f32x4*)di, (const f32x4*)dact, B, L, E / 4, (f32x4*)dpre};
  const int64_t n = (int64_t)B * (L + 2) * a.ev;
  hipLaunchKernelGGL(curator_pool_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return pxr_check_launch("pxr_curator_pool_bwd_f32");
}
