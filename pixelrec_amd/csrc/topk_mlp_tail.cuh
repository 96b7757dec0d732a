// topk_mlp_tail.cuh -- what follows the first hidden layer in the fused top-k kernels that score with a small MLP (din.hip,
// widedeep.hip): a tile of 128 items x the first layer's activations in LDS, an optional second hidden layer on the fp32-operand
// MFMA against W2 held in LDS, and the dot product with the last layer's weights, one thread per item.  The first layer, the
// biases' meaning and every barrier stay in the kernels; the activation is a functor (float -> float) of the kernel's model.
#pragma once
#include "gemm_f32.cuh"

namespace pxr {

constexpr int MT_BM = 128;                     // items per tile; the hidden widths are at most 128 as well
constexpr int MT_LD = 132;                     // LDS row stride of the activation tile and of W2 (16-byte rows for ds_read_b128)
constexpr int MT_TILE = MT_BM * MT_LD;
static_assert(MT_TILE >= 2 * GemmCfg<MT_BM, 128, true, true>::STAGE, "the activation tile overlays the staging buffers");

// once per workgroup: W2 -> w2s [128][MT_LD], zero outside [h2][h1]; the last layer's weights -> wls [128], zero beyond h_last;
// b2 -> b2s [128].  TWO = two hidden layers.
template <bool TWO>
__device__ __forceinline__ void mlp_tail_stage(float* w2s, float* wls, float* b2s, const float* w2, const float* b2, const float* wl,
                                               int h1, int h2, int tid) {
  if constexpr (TWO) {
    for (int e = tid; e < MT_TILE; e += GEMM_THREADS) {
      const int j2 = e / MT_LD, k = e - j2 * MT_LD;
      w2s[e] = (j2 < h2 && k < h1) ? w2[j2 * h1 + k] : 0.f;
    }
  }
  if (tid < 128) {
    wls[tid] = tid < (TWO ? h2 : h1) ? wl[tid] : 0.f;
    b2s[tid] = (TWO && tid < h2) ? b2[tid] : 0.f;
  }
}

// second layer on the MFMA: the wave owns 32 items x every column block of h2; lanes 0-31 feed k 0..3, lanes 32-63 k 4..7.
// ksteps = ceil(h1 / 8) -- the k loop may read past h1 and relies on the zero padding of tile and w2s --, nb2 = ceil(h2 / 32),
// r = lane & 31, hh = lane >> 5: the kernel computes them once (recomputed here, the two-layer kernels took up to 24 more VGPRs).
__device__ __forceinline__ void mlp_tail_layer2(f32x16 (&acc2)[4], const float* tile, const float* w2s, int ksteps, int nb2, int wave,
                                                int r, int hh) {
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc2[jb][e] = 0.f;
  const float* arow = tile + (wave * 32 + r) * MT_LD + hh * 4;
  const float* brow = w2s + r * MT_LD + hh * 4;
  for (int k8 = 0; k8 < ksteps; ++k8) {
    const float4 av = *reinterpret_cast<const float4*>(arow + k8 * 8);
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      if (jb < nb2) {
        const float4 bv = *reinterpret_cast<const float4*>(brow + jb * 32 * MT_LD + k8 * 8);
        acc2[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv.x, acc2[jb], 0, 0, 0);
        acc2[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv.y, acc2[jb], 0, 0, 0);
        acc2[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv.z, acc2[jb], 0, 0, 0);
        acc2[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv.w, acc2[jb], 0, 0, 0);
      }
    }
  }
}
// ... and, once every wave has read the first layer's activations (the kernel's barrier), act(acc2 + b2) back into the tile
template <class Act>
__device__ __forceinline__ void mlp_tail_layer2_store(float* tile, const f32x16 (&acc2)[4], const float* b2s, int nb2, int wave,
                                                      int r, int hh, Act act) {
#pragma unroll
  for (int jb = 0; jb < 4; ++jb) {
    if (jb < nb2) {
      const int col = jb * 32 + r;
      const float bb = b2s[col];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int rl = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
        tile[rl * MT_LD + col] = act(acc2[jb][e] + bb);
      }
    }
  }
}

// sum_j wls[j] row[j] over the hl last activations of one item, started at column jstart = tid % hl and wrapped around: every
// item thread starts at another column, so the reads of wls and of the tile rows do not collide on LDS banks
__device__ __forceinline__ float mlp_tail_dot(const float* wls, const float* row, int hl, int jstart) {
  float s = 0.f;
  int j = jstart;
  for (int jj = 0; jj < hl; ++jj) {
    s += wls[j] * row[j];
    j = j + 1 == hl ? 0 : j + 1;
  }
  return s;
}

}  // namespace pxr
