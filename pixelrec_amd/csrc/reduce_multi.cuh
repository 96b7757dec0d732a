// reduce_multi.cuh -- the small second-stage reductions that close a backward pass, as __device__ bodies, so that the launch
// that runs them can be either their own kernel (reduce_partials_multi_kernel, layernorm.hip; bpr_reduce_kernel, bpr_loss.hip)
// or a launch that runs anyway: the segment sums of the table gradient carry them as a RIDER (embed_grad.hip) -- extra
// workgroups appended to the grid that share no byte with the carrier's.  One body each => the same association and the same
// bits wherever it runs.
#pragma once
#include "pxr_common.h"

#ifdef __HIPCC__
// up to 16 independent partial buffers: out_a[i][c] (c < split[i]) / out_b[i][c - split[i]] = sum_p part[i][p][c], c < N[i]
struct MultiReduce {
  const float* part[16]; float* out_a[16]; float* out_b[16];
  int P[16], N[16], split[16], blk_begin[17];   // blk_begin: first column group (PXR_RED_CX columns) of problem i; [n]: their count
  int n;
  int64_t* bump;   // optional device counter incremented by one (e.g. the dropout step counter: this is the last
                   // kernel of a backward pass that could read it, so the separate 1-thread launch is saved)
};

// One column group of the problem set by one 256-thread group: grp = index of the column group in [0, blk_begin[n]), tid =
// the thread's index inside its group, red = the group's own LDS tile.  Per column pxr_strided_column_sum +
// pxr_combine_row_lanes (pxr_common.h), as the single form.  EVERY thread of the workgroup must call this (one barrier inside): a
// group with grp >= blk_begin[n] (the odd half of a two-group workgroup) reads and writes nothing.
__device__ __forceinline__ void pxr_reduce_multi_group(const MultiReduce& m, int grp, int tid, float (&red)[PXR_RED_CY][PXR_RED_CX + 1]) {
  int pi = 0;
  for (int i = 1; i < m.n; ++i)
    if (grp >= m.blk_begin[i]) pi = i;
  const bool live = grp < m.blk_begin[m.n];
  const float* part = m.part[pi];
  const int P = m.P[pi], N = live ? m.N[pi] : 0;
  const int tx = tid % PXR_RED_CX, ty = tid / PXR_RED_CX;
  const int col = (grp - m.blk_begin[pi]) * PXR_RED_CX + tx;
  const float s = (col < N) ? pxr_strided_column_sum(part, P, N, col, ty) : 0.f;
  const float v = pxr_combine_row_lanes(s, red, tx, ty);
  if (ty == 0 && col < N) {
    if (col < m.split[pi]) m.out_a[pi][col] = v;
    else m.out_b[pi][col - m.split[pi]] = v;
  }
  if (m.bump && grp == 0 && tid == 0) m.bump[0] += 1;
}

// loss = (1/B) * sum_b ( sum_t lossrow[b,t] ), fixed order, by the first 256 threads of a workgroup (tid = threadIdx.x; red: 256
// floats of LDS).  EVERY thread of the workgroup must call this (barriers inside): threads beyond 255 add nothing.
__device__ __forceinline__ void pxr_bpr_reduce_block(const float* __restrict__ lossrow, int B, int L, float* __restrict__ loss,
                                                     float* red, int tid) {
  if (tid < 256) {
    float s = 0.f;
    for (int b = tid; b < B; b += 256) {
      const float* row = lossrow + (int64_t)b * L;
      float sb = 0.f;
      int t = 0;
      for (; t + 8 <= L; t += 8) {   // 8 independent loads per round trip, added in position order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = row[t + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) sb += v[u];
      }
      for (; t < L; ++t) sb += row[t];
      s += sb;
    }
    red[tid] = s;
  }
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) loss[0] = red[0] / (float)B;
}

// ---- the rider --------------------------------------------------------------------------------------------------------------
// What a carrier launch of 512-thread workgroups runs on `blocks` workgroups appended to its grid: rider block j < red_blocks
// runs column groups 2j and 2j + 1 of `m` on its two 256-thread halves (an odd count leaves the last half idle); the block
// after them, when loss != null, runs the loss sum on its first half.  blocks == 0: no rider.
struct TailRider {
  MultiReduce m;
  const float* lossrow; float* loss;
  int B, L;
  int red_blocks, blocks;
};
constexpr int PXR_RIDER_THREADS = 512;
constexpr int PXR_RIDER_LDS = 2 * PXR_RED_CY * (PXR_RED_CX + 1) * 4;   // bytes of LDS a rider block needs (>= 256 floats)
static_assert(PXR_RIDER_LDS >= 256 * 4, "the loss sum's 256 floats fit the two reduction tiles");

// rb = index of the rider block among the rider blocks (block-uniform); lds: PXR_RIDER_LDS bytes, 16-byte aligned
__device__ __forceinline__ void pxr_tail_rider_block(const TailRider& r, int rb, void* lds) {
  if (rb < r.red_blocks) {
    const int half = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 8);
    auto* red = reinterpret_cast<float (*)[PXR_RED_CY][PXR_RED_CX + 1]>(lds);
    pxr_reduce_multi_group(r.m, 2 * rb + half, (int)threadIdx.x & 255, red[half]);
  } else if (r.loss) {
    pxr_bpr_reduce_block(r.lossrow, r.B, r.L, r.loss, reinterpret_cast<float*>(lds), (int)threadIdx.x);
  }
}

// Host side (layernorm.hip): the descriptor of include/pxr.h (pxr_tail_rider, passed as const void*) checked and turned into the
// kernel argument.  what: the entry point's name for the error message.  rider == null: out->blocks = 0.
int pxr_tail_rider_prepare(const void* rider, const char* what, TailRider* out);
#endif
