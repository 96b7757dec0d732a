// gemm_f32.cuh -- LDS-tiled fp32 GEMM main loop on the gfx950 f32-input MFMA (v_mfma_f32_32x32x2_f32).
//
// Why f32 MFMA: the parity bar is +-1e-4 on logits / +-1e-5 on post-step parameters against the fp32
// reference (SURVEY.md §7 hard part 1).  v_mfma_f32_32x32x2_f32 is bit-for-bit an fp32 fmaf chain and runs
// at the fp32 vector peak (157 TFLOP/s) from ONE wave per SIMD; gfx950 has no xf32/TF32.
//
// Computes C[M,N] = A_op[M,K] * B_op[K,N] for operands stored either
//   "KC" (k-contiguous):  A as [M][K] row-major (lda = row stride),  B as [N][K] row-major  (nn.Linear weight)
//   "XC" (x-contiguous):  A as [K][M] row-major,                      B as [K][N] row-major
// which covers   Y = X W^T            (KC,KC)   reference layers.py:586-588,613,666,669 and sasrec.py:112
//                dX = dY W            (KC,XC)   autograd of the above
//                dW = dY^T X          (XC,XC)   autograd of the above (reduction over tokens, split-K)
//
// Tiling: 256 threads = 4 waves arranged 2x2; block tile BM x BN, K step BK = 32; each wave owns
// (BM/2)x(BN/2) made of 32x32 MFMA blocks.  LDS images need no transposes in either flavour:
//   KC operand -> LDS [row][k], 32 floats per row, 16-byte slots XOR-swizzled by the row (kc_slot: conflict-free
//                 ds_write_b128 / ds_read_b128 without padding);
//                 a lane reads 4 consecutive k; lanes 0-31 take k 0..3, lanes 32-63 take k 4..7 of the
//                 8-wide k sub-step, so register t feeds MFMA t with k = 4*(lane>>5)+t on BOTH operands.
//   XC operand -> LDS [k][x] with row stride BM (or BN) floats; per MFMA one ds_read_b32 at
//                 [4*(lane>>5)+t][x0 + (lane&31)] (32 consecutive floats per half-wave: conflict-free).
// Double-buffered: global loads for tile kt+1 are issued into registers before the MFMAs of tile kt and
// written to the other LDS buffer afterwards; one barrier per K tile.
#pragma once
#include "pxr_common.h"
#include "gemm_epi.cuh"

namespace pxr {

constexpr int GEMM_BK = 32;
constexpr int GEMM_THREADS = 256;

// KW = number of wave groups that split the k-steps of each K tile between them (intra-workgroup split-K): KW=2
// doubles the waves per output tile, which is what hides the LDS/global latency bubbles when a GEMM has too few
// output tiles to fill the chip (M = B*L = 3200 tokens); the KW partial accumulators are added through LDS.
template <int BM, int BN, bool A_KC, bool B_KC, int KW = 1, int FINE = 0>
struct GemmCfg {
  static constexpr int BK = GEMM_BK;
  // wave grid of one k-group: WGM x 2.  BM = 32 tiles use one wave row; with KW = 2 that is still a 256-thread
  // workgroup, but each output tile is half as large: twice as many, independently synchronised workgroups per CU --
  // what overlaps one workgroup's barrier / LDS bubbles when a GEMM has few tiles (waves of ONE workgroup run in
  // lockstep between barriers, so more waves per workgroup do not help: measured with the 64x64 KW=2 tile).
  // FINE = 1: every wave owns ONE 32x32 block of the tile (a 128x128 tile = 16 waves).  The 64x64 kernels turned out
  // to be bound by L2 -> LDS traffic (16 flop per byte staged: ~6 TB/s at 94 TFLOP/s), not by occupancy; a big tile
  // cut into many small wave tiles halves that traffic while keeping the same number of waves in flight.
  // FINE = 2: 64x32 per wave (a 128x128 tile = 8 waves, 2 x 4): half the accumulator registers of the 64x64 wave tile.
  static constexpr int WGM = FINE == 1 ? BM / 32 : (FINE == 2 ? BM / 64 : ((BM >= 64) ? 2 : 1));
  static constexpr int WGN = FINE ? BN / 32 : 2;
  static constexpr int G = WGM * WGN;
  static constexpr int NT = 64 * G * KW;
  static constexpr int LDA = A_KC ? BK : BM;   // KC tiles are XOR-swizzled, not padded (see kc_slot)
  static constexpr int LDB = B_KC ? BK : BN;
  static constexpr int A_STAGE = (A_KC ? BM : BK) * LDA;  // floats
  static constexpr int B_STAGE = (B_KC ? BN : BK) * LDB;
  static constexpr int STAGE = A_STAGE + B_STAGE;
  static constexpr int LDS_BYTES = 2 * STAGE * 4;
  static constexpr int WM = BM / WGM, WN = BN / WGN;
  static constexpr int TM = WM / 32, TN = WN / 32;
  static constexpr int A_LD4 = BM * BK / 4 / NT;  // float4 loads per thread per tile
  static constexpr int B_LD4 = BN * BK / 4 / NT;
  static_assert(A_LD4 >= 1 && B_LD4 >= 1, "tile too small for this many threads");
  static_assert(BM % 32 == 0 && BN % 64 == 0, "tile must be a multiple of 32 x 64");
  struct Acc {
    f32x16 v[TM][TN];
  };
};

// ---- global -> register tile fetch (zero-filled outside the matrix) ------------------------------------
// Through buffer loads: the hardware bounds check returns 0 for lanes whose offset lies outside the descriptor, so
// ragged edges need no branch (a divergent branch around a load makes the compiler drain ALL outstanding loads --
// s_waitcnt vmcnt(0) -- at the top of every K tile, which defeats any prefetching).  Descriptors are built from
// block-uniform values only (kernel arguments, blockIdx-derived tile origins, the K-tile counter).
typedef __amdgpu_buffer_rsrc_t bufrsrc;
__device__ __forceinline__ bufrsrc make_rsrc(const float* base, int64_t bytes) {
  const int nb = bytes > 0x7FFFFFF0ll ? 0x7FFFFFF0 : (bytes < 0 ? 0 : (int)bytes);
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, nb, 0x00020000);
}
__device__ __forceinline__ float4 buf_ld16(bufrsrc rs, unsigned byte_off) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, byte_off, 0, 0);
  return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}
constexpr unsigned BUF_OOB = 0xFFFFFFFFu;

// KC operand: matrix [X][K] (row stride ld); `rs` starts at the tile's first row, rows_left = X - x0
template <int BX, int NLD, int NT>
__device__ __forceinline__ void fetch_kc(float4 (&r)[NLD], bufrsrc rs, int ld, int rows_left, int k0, int kend,
                                         int tid) {
#pragma unroll
  for (int p = 0; p < NLD; ++p) {
    const int f = tid + p * NT;  // float4 index in tile: row = f/8, q = f%8
    const int row = f >> 3, q = f & 7;
    const int gk = k0 + q * 4;
    const bool ok = row < rows_left && gk < kend;
    r[p] = buf_ld16(rs, ok ? (unsigned)(row * ld + gk) * 4u : BUF_OOB);
  }
}
// A KC tile is [row][32 floats] = 8 sixteen-byte slots per row, UNPADDED; logical slot q of `row` lives in physical slot
// q ^ ((row >> 1) & 7).  A 16-lane group of a ds_read_b128 / ds_write_b128 then touches 16 distinct 16-byte bank
// groups (rows r, r+1 differ in the 128-byte half, rows r, r+2 in the slot), i.e. the same conflict-freedom as a
// 36-float padded stride at 32 KB instead of 36.9 KB per 64x64 double-buffered tile: FIVE workgroups per CU instead of
// four, so the 1200-tile QKV GEMM of the training step is resident in one round.
__device__ __forceinline__ int kc_slot(int row, int q) { return (q ^ ((row >> 1) & 7)) * 4; }

template <int BX, int NLD, int NT>
__device__ __forceinline__ void stash_kc(const float4 (&r)[NLD], float* lds, int tid) {
#pragma unroll
  for (int p = 0; p < NLD; ++p) {
    const int f = tid + p * NT;
    const int row = f >> 3, q = f & 7;
    *reinterpret_cast<float4*>(lds + row * GEMM_BK + kc_slot(row, q)) = r[p];
  }
}
// XC operand: matrix [K][X] (row stride ld); `rs` starts at element [k0][x0], krows_left = kend - k0,
// cols_left = X - x0
template <int BX, int NLD, int NT>
__device__ __forceinline__ void fetch_xc(float4 (&r)[NLD], bufrsrc rs, int ld, int krows_left, int cols_left,
                                         int tid) {
  constexpr int Q = BX / 4;  // float4 per k row
#pragma unroll
  for (int p = 0; p < NLD; ++p) {
    const int f = tid + p * NT;
    const int kk = f / Q, q = f % Q;
    const bool ok = kk < krows_left && q * 4 < cols_left;
    r[p] = buf_ld16(rs, ok ? (unsigned)(kk * ld + q * 4) * 4u : BUF_OOB);
  }
}
template <int BX, int NLD, int NT>
__device__ __forceinline__ void stash_xc(const float4 (&r)[NLD], float* lds, int tid) {
  constexpr int Q = BX / 4;
#pragma unroll
  for (int p = 0; p < NLD; ++p) {
    const int f = tid + p * NT;
    const int kk = f / Q, q = f % Q;
    *reinterpret_cast<float4*>(lds + kk * BX + q * 4) = r[p];
  }
}

// ---- the main loop ---------------------------------------------------------------------------------------
// acc[bi][bj] element `reg` of lane l is C[m0 + wm*WM + bi*32 + (reg&3) + 8*(reg>>2) + 4*(l>>5)]
//                                         [n0 + wn*WN + bj*32 + (l&31)]          (gfx950 32x32 C/D map)
// CS (only with an XC A operand): additionally accumulate, per thread, the sum over k of the A float4s it stages
// (column sums of the stored [K][M] matrix = bias gradient when A = dY) into *cs; the caller reduces across threads.
// PD = prefetch depth: tiles kt+1 .. kt+PD are in flight (global -> registers) while tile kt is multiplied.  A 64x64
// tile spends only ~0.43 us of MFMA time per K tile, far less than a global round trip, so with PD = 1 a workgroup
// that is alone on its CU (M = B*L = 3200 tokens => ~1.5 workgroups per CU) stalls on every K tile; PD = 3..4 keeps
// enough loads in flight (16 VGPRs per slot at 64x64).  LDS stays double-buffered: slot (kt+1) % PD is written to
// the other buffer while tile kt is read.
// DUAL: two accumulator sets per wave, used by alternate 8-wide k sub-steps and added at the end.  A wave tile of ONE
// 32x32 block is a single dependent MFMA chain: whatever the wave issues between two MFMAs of that chain (fragment
// reads, waits, the barrier) delays the next MFMA by more than its own issue time (MI355X_MICROARCH.md: +43 cycles
// for the first extra issue slot between MFMAs on the same accumulator).  With two chains the gap of one is covered by
// the other.  (Summation order changes: even and odd sub-steps are summed separately, then added.)
// A_GATHER (KC A operand only): row m of the A operand is row a_rows[m] of the matrix at A (a negative entry: a row of zeros),
// a_rows holds at least m0 + BM entries and the gathered matrix is smaller than 2 GiB (32-bit buffer offsets).
template <int BM, int BN, bool A_KC, bool B_KC, bool CS = false, int KW = 1, int PD = 2, int ST = 2, int FINE = 0,
          bool DUAL = false, bool A_GATHER = false>
__device__ __forceinline__ void gemm_mainloop(typename GemmCfg<BM, BN, A_KC, B_KC, KW, FINE>::Acc& accs,
                                              const float* __restrict__ A, int64_t lda,
                                              const float* __restrict__ B, int64_t ldb, int M, int N,
                                              int kbeg, int kend, int m0, int n0, float* smem,
                                              float4* cs = nullptr, const int* __restrict__ a_rows = nullptr) {
  using Cfg = GemmCfg<BM, BN, A_KC, B_KC, KW, FINE>;
  constexpr int NT = Cfg::NT;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wk = wave / Cfg::G, w4 = wave % Cfg::G;
  const int wm = w4 / Cfg::WGN, wn = w4 % Cfg::WGN;
  const int h = lane >> 5, r = lane & 31;
  auto& acc = accs.v;
  f32x16 acc2[DUAL ? Cfg::TM : 1][DUAL ? Cfg::TN : 1];

#pragma unroll
  for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        acc[i][j][e] = 0.f;
        if constexpr (DUAL) acc2[i][j][e] = 0.f;
      }

  float4 ra[PD][Cfg::A_LD4], rb[PD][Cfg::B_LD4];
  const int nk = (kend - kbeg + GEMM_BK - 1) / GEMM_BK;
  if (nk <= 0) return;

  // descriptors of the k-contiguous operands cover the tile's rows for the whole K range; the x-contiguous ones are
  // re-based per K tile (32-bit offsets stay small however long the token reduction is)
  bufrsrc rsA = make_rsrc(A, 0), rsB = make_rsrc(B, 0);
  if constexpr (A_KC && !A_GATHER) rsA = make_rsrc(A + (int64_t)m0 * lda, (int64_t)(M - m0) * lda * 4);
  int arow[A_GATHER ? Cfg::A_LD4 : 1];
  if constexpr (A_GATHER) {
    static_assert(!A_GATHER || A_KC, "row gather is built for a k-contiguous A operand");
    rsA = make_rsrc(A, 0x7FFFFFF0ll);
#pragma unroll
    for (int p = 0; p < Cfg::A_LD4; ++p) arow[p] = a_rows[m0 + ((tid + p * NT) >> 3)];
  }
  if constexpr (B_KC) rsB = make_rsrc(B + (int64_t)n0 * ldb, (int64_t)(N - n0) * ldb * 4);
  auto fetch = [&](int kt, float4 (&fa)[Cfg::A_LD4], float4 (&fb)[Cfg::B_LD4]) {
    const int k0 = kbeg + kt * GEMM_BK;
    if constexpr (A_GATHER) {
#pragma unroll
      for (int p = 0; p < Cfg::A_LD4; ++p) {
        const int gk = k0 + ((tid + p * NT) & 7) * 4;
        fa[p] = buf_ld16(rsA, (arow[p] >= 0 && gk < kend) ? ((unsigned)arow[p] * (unsigned)lda + (unsigned)gk) * 4u : BUF_OOB);
      }
    } else if constexpr (A_KC) {
      fetch_kc<BM, Cfg::A_LD4, NT>(fa, rsA, (int)lda, M - m0, k0, kend, tid);
    } else {
      const bufrsrc rs = make_rsrc(A + (int64_t)k0 * lda + m0, ((int64_t)(kend - k0) * lda - m0) * 4);
      fetch_xc<BM, Cfg::A_LD4, NT>(fa, rs, (int)lda, kend - k0, M - m0, tid);
    }
    if constexpr (CS) {
      static_assert(!A_KC, "column sums are taken over an x-contiguous A operand");
#pragma unroll
      for (int p = 0; p < Cfg::A_LD4; ++p) { cs->x += fa[p].x; cs->y += fa[p].y; cs->z += fa[p].z; cs->w += fa[p].w; }
    }
    if constexpr (B_KC) {
      fetch_kc<BN, Cfg::B_LD4, NT>(fb, rsB, (int)ldb, N - n0, k0, kend, tid);
    } else {
      const bufrsrc rs = make_rsrc(B + (int64_t)k0 * ldb + n0, ((int64_t)(kend - k0) * ldb - n0) * 4);
      fetch_xc<BN, Cfg::B_LD4, NT>(fb, rs, (int)ldb, kend - k0, N - n0, tid);
    }
  };
  auto stash = [&](int buf, const float4 (&fa)[Cfg::A_LD4], const float4 (&fb)[Cfg::B_LD4]) {
    float* sa = smem + buf * Cfg::STAGE;
    float* sb = sa + Cfg::A_STAGE;
    if constexpr (A_KC) stash_kc<BM, Cfg::A_LD4, NT>(fa, sa, tid);
    else stash_xc<BM, Cfg::A_LD4, NT>(fa, sa, tid);
    if constexpr (B_KC) stash_kc<BN, Cfg::B_LD4, NT>(fb, sb, tid);
    else stash_xc<BN, Cfg::B_LD4, NT>(fb, sb, tid);
  };
  // fragments of one 8-wide k sub-step: a[i][t] / b[j][t] feed MFMA t (see the layout notes at the top)
  struct Frag {
    float a[Cfg::TM][4], b[Cfg::TN][4];
  };
  constexpr int NS = GEMM_BK / 8 / KW;   // sub-steps per K tile for this wave group
  static_assert(NS % 2 == 0, "fragment double-buffering needs an even number of sub-steps");
  auto read_frag = [&](Frag& f, int buf, int ks0) {
    const float* sa = smem + buf * Cfg::STAGE;
    const float* sb = sa + Cfg::A_STAGE;
    const int ks = ks0 * KW + (KW > 1 ? wk : 0);
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i) {
      const int row = wm * Cfg::WM + i * 32 + r;
      if constexpr (A_KC) {
        const float4 v = *reinterpret_cast<const float4*>(sa + row * Cfg::LDA + kc_slot(row, ks * 2 + h));
        f.a[i][0] = v.x; f.a[i][1] = v.y; f.a[i][2] = v.z; f.a[i][3] = v.w;
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) f.a[i][t] = sa[(ks * 8 + h * 4 + t) * Cfg::LDA + row];
      }
    }
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j) {
      const int col = wn * Cfg::WN + j * 32 + r;
      if constexpr (B_KC) {
        const float4 v = *reinterpret_cast<const float4*>(sb + col * Cfg::LDB + kc_slot(col, ks * 2 + h));
        f.b[j][0] = v.x; f.b[j][1] = v.y; f.b[j][2] = v.z; f.b[j][3] = v.w;
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) f.b[j][t] = sb[(ks * 8 + h * 4 + t) * Cfg::LDB + col];
      }
    }
  };
  auto mfma = [&](const Frag& f, int t0, int t1) {
#pragma unroll
    for (int t = t0; t < t1; ++t)
#pragma unroll
      for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
        for (int j = 0; j < Cfg::TN; ++j) {
          if (DUAL && (t & 1))
            acc2[DUAL ? i : 0][DUAL ? j : 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[i][t], f.b[j][t], acc2[DUAL ? i : 0][DUAL ? j : 0], 0, 0, 0);
          else
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[i][t], f.b[j][t], acc[i][j], 0, 0, 0);
        }
  };

  // tile j lives in register slot j % PD.  Fetches past the last K tile are issued unconditionally: every lane is
  // out of range, so they move no data and return zeros -- and a straight-line loop body lets the compiler count
  // outstanding loads exactly (s_waitcnt vmcnt(n) for the slot being written instead of draining everything).
#pragma unroll
  for (int s = 0; s < PD; ++s) fetch(s, ra[s], rb[s]);
  stash(0, ra[0], rb[0]);
  __syncthreads();
  Frag fr[2];
  read_frag(fr[0], 0, 0);

  // Software pipeline inside the wave.  Instructions issue in order and a wave can run at most one MFMA ahead of the
  // matrix pipe, so whatever should overlap with MFMA execution has to be ISSUED before those MFMAs; the
  // sched_barriers pin that order (left alone, the scheduler moves the LDS reads behind the MFMAs they should
  // overlap with):  fragments of sub-step q+1 are read before sub-step q multiplies; the next tile is written to the
  // other LDS buffer before the last sub-step; the barrier sits in the MIDDLE of the last sub-step and the first
  // fragment read of the next tile follows it immediately, so both run under the remaining MFMAs.
  // ST = 2: the next tile goes to the OTHER LDS buffer (one barrier per K tile).  ST = 1: a single LDS buffer (half the
  // LDS, so twice the resident workgroups per CU): two barriers per K tile -- everybody finished reading, everybody
  // finished writing -- whose latency is covered by the other workgroups' waves instead of by a second buffer.
  for (int kt0 = 0; kt0 < nk; kt0 += PD) {
#pragma unroll
    for (int s = 0; s < PD; ++s) {
      const int kt = kt0 + s;
      if (kt < nk) {   // block-uniform
        const int buf = (ST == 2) ? (kt & 1) : 0;
        const int nxt = (ST == 2) ? (buf ^ 1) : 0;
        fetch(kt + PD, ra[s], rb[s]);   // slot s held tile kt, which already sits in LDS
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q + 1 < NS; ++q) {
          read_frag(fr[(q + 1) & 1], buf, q + 1);
          __builtin_amdgcn_sched_barrier(0);
          mfma(fr[q & 1], 0, 4);
          __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (ST == 2) {
          stash(nxt, ra[(s + 1) % PD], rb[(s + 1) % PD]);   // (zeros after the last tile)
          __builtin_amdgcn_sched_barrier(0);
          mfma(fr[(NS - 1) & 1], 0, 2);
          __syncthreads();
        } else {
          mfma(fr[(NS - 1) & 1], 0, 2);
          __syncthreads();                                    // all fragments of tile kt are in registers
          stash(nxt, ra[(s + 1) % PD], rb[(s + 1) % PD]);
          __syncthreads();
        }
        read_frag(fr[0], nxt, 0);
        __builtin_amdgcn_sched_barrier(0);
        mfma(fr[(NS - 1) & 1], 2, 4);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  __syncthreads();   // the staging LDS is reused by the callers' epilogues
  if constexpr (DUAL) {
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
      for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] += acc2[i][j][e];
  }
  if constexpr (KW > 1) {
    // add the partial accumulators of wave group 1 into wave group 0 through LDS (the staging buffers are free:
    // the loop ended with a barrier).  Layout [w4][element][lane] => conflict-free 4-byte accesses.
    static_assert(KW == 2, "intra-workgroup split-K is built for 2 wave groups");
    constexpr int NE = Cfg::TM * Cfg::TN * 16;
    static_assert(Cfg::G * NE * 64 <= ST * Cfg::STAGE, "accumulator exchange does not fit in the staging LDS");
    float* ex = smem + (w4 * NE) * 64 + lane;
    if (wk == 1) {
#pragma unroll
      for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
        for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) ex[((i * Cfg::TN + j) * 16 + e) * 64] = acc[i][j][e];
    }
    __syncthreads();
    if (wk == 0) {
#pragma unroll
      for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
        for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][j][e] += ex[((i * Cfg::TN + j) * 16 + e) * 64];
    }
  }
}

// Batched launch: grid.z = batch index z; operand offsets (in floats) = (z / nb2) * x1 + (z % nb2) * x2 -- two levels, so
// that "image n, head h" of a packed [n, T, 3, heads, d] projection is addressed without copies.
struct GemmBatch {
  int nb2;
  int64_t a1, a2, b1, b2, c1, c2;
  int act;      // EPI_BIAS_ACT_GRAD: which activation (ACT_*)
};

// ---- epilogue pieces shared by the tile-per-workgroup kernel and the stream-K kernel ---------------------------------
// DIRECT: the epilogue reads `aux` from memory itself instead of from registers filled before the main loop (kernels
// that have no registers to spare)
template <class Cfg, int EPI, bool DIRECT = false>
struct AuxRegs {
  static constexpr bool R = EpiTraits<EPI>::READS_AUX && !DIRECT;
  float v[R ? Cfg::TM : 1][R ? Cfg::TN : 1][R ? 16 : 1];
};
// where this lane's accumulator elements live in the output tile
struct LanePos {
  int wm, wn, h, r;
};
template <class Cfg>
__device__ __forceinline__ LanePos lane_pos() {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  return LanePos{(wave % Cfg::G) / Cfg::WGN, (wave % Cfg::G) % Cfg::WGN, lane >> 5, lane & 31};
}
// epilogue operands that are READ (residual-branch gradient / saved pre-activation) are fetched before the main
// loop: the loads complete under the MFMAs instead of stalling every wave after its last one
template <class Cfg, int EPI, bool DIRECT = false>
__device__ __forceinline__ void epi_prefetch_aux(AuxRegs<Cfg, EPI, DIRECT>& ar, const float* __restrict__ aux, int64_t ldaux, int M,
                                                 int N, int m0, int n0, const LanePos p) {
  if constexpr (EpiTraits<EPI>::READS_AUX && !DIRECT) {
#pragma unroll
    for (int j = 0; j < Cfg::TN; ++j) {
      const int col = n0 + p.wn * Cfg::WN + j * 32 + p.r;
#pragma unroll
      for (int i = 0; i < Cfg::TM; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = m0 + p.wm * Cfg::WM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * p.h;
          ar.v[i][j][e] = (col < N && row < M) ? aux[(int64_t)row * ldaux + col] : 0.f;
        }
    }
  }
}
template <class Cfg, int EPI, bool DIRECT = false>
__device__ __forceinline__ void epi_store(const typename Cfg::Acc& accs, const AuxRegs<Cfg, EPI, DIRECT>& ar, float* __restrict__ C,
                                          int64_t ldc, int M, int N, const float* __restrict__ bias,
                                          float* __restrict__ aux, int64_t ldaux, int m0, int n0, const LanePos p, int act) {
  const auto& acc = accs.v;
#pragma unroll
  for (int j = 0; j < Cfg::TN; ++j) {
    const int col = n0 + p.wn * Cfg::WN + j * 32 + p.r;
    if (col >= N) continue;
    float bv = 0.f;
    if constexpr (EpiTraits<EPI>::HAS_BIAS) bv = bias[col];
#pragma unroll
    for (int i = 0; i < Cfg::TM; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + p.wm * Cfg::WM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * p.h;
        if (row >= M) continue;
        float av = 0.f, ao;
        if constexpr (EpiTraits<EPI>::READS_AUX) av = DIRECT ? aux[(int64_t)row * ldaux + col] : ar.v[DIRECT ? 0 : i][DIRECT ? 0 : j][DIRECT ? 0 : e];
        const float v = epi_elem<EPI>(acc[i][j][e], bv, av, ao, act);
        if constexpr (EpiTraits<EPI>::WRITES_AUX) aux[(int64_t)row * ldaux + col] = ao;
        C[(int64_t)row * ldc + col] = v;
      }
    }
  }
}

constexpr int DW_MAX = 16;
struct DwProblem {
  const float* dy; const float* x; float* dW; float* db;
  int M, N, K;        // tokens, out features, in features
  int tile_begin, tiles_m;
};
struct DwGroup {
  DwProblem p[DW_MAX];
  int n, total_tiles;
};


// ---- entry points of gemm_b3.hip (the same products on the bf16 matrix pipe, gemm_b3.cuh) used by gemm_f32.hip ---------
// tile: 64 (64x64, 4 waves) or 1281 (128x128, 16 waves).  Same argument meaning as gemm_kernel's launch.
int gemm_b3_launch(int a_kc, int b_kc, int epilogue, int tile, const float* A, int64_t lda, const float* B, int64_t ldb,
                   float* C, int64_t ldc, int M, int N, int K, const float* bias, float* aux, int64_t ldaux, int splits,
                   int ksplit_len, int64_t split_stride, const GemmBatch& bt, int batch, hipStream_t st);
int grouped_dw_b3_launch(const DwGroup& g, hipStream_t st);
}  // namespace pxr
