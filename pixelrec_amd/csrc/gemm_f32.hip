// gemm_f32.hip -- fp32 MFMA GEMM entry points: nn.Linear forward / input-grad / weight-grad, plus the
// deterministic column reductions used for bias / LayerNorm-affine / position-embedding gradients.
//
// Reference call sites replaced (all are ATen -> cuBLAS sgemm in the reference):
//   layers.py:586-588 (query/key/value), :613 (dense), :666 (dense_1 + erf-GELU :651-660,667), :669 (dense_2),
//   sasrec.py:112 (full-catalog scoring, un-fused form) and the autograd transposes of all of them.
#include "gemm_f32.cuh"

#include <cstdlib>
#include <mutex>
#include <unordered_map>

namespace pxr {

template <int BM, int BN, bool A_KC, bool B_KC, int EPI, int KW = 1, int PD = 1, int ST = 2, int FINE = 0, bool DUAL = false>
__global__ void __launch_bounds__((GemmCfg<BM, BN, A_KC, B_KC, KW, FINE>::NT))
gemm_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb,
            float* __restrict__ C, int64_t ldc, int M, int N, int K, const float* __restrict__ bias,
            float* __restrict__ aux, int64_t ldaux, int tiles_m, int tiles_n, int ksplit_len,
            int64_t split_stride, int n_fastest, GemmBatch bt) {
  using Cfg = GemmCfg<BM, BN, A_KC, B_KC, KW, FINE>;
  __shared__ __attribute__((aligned(16))) float smem[ST * Cfg::STAGE];
  if (bt.nb2 > 0) {   // batched launch (block-uniform)
    const int z1 = blockIdx.z / bt.nb2, z2 = blockIdx.z % bt.nb2;
    A += z1 * bt.a1 + z2 * bt.a2;
    B += z1 * bt.b1 + z2 * bt.b2;
    C += z1 * bt.c1 + z2 * bt.c2;
  }

  // Each XCD (private 4 MB L2) works on one contiguous chunk of the tile sequence, so the ORDER of that sequence decides
  // what every XCD pulls over the fabric: m fastest => an XCD owns whole B panels and streams ALL of A (8|A| + |B| in
  // total: right for the scoring GEMM, 1024 users x 400 K table rows); n fastest => an XCD owns a band of A rows and
  // reads all of B (|A| + 8|B|: right for the training step, where A = 3200 tokens x K is 2-6x larger than the weight.
  // PMC FETCH_SIZE of the dX GEMM [3200,1536]x[1536,512]: 137 MB with m fastest vs 29 MB algorithmic).
  const int t = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int tm = n_fastest ? t / tiles_n : t % tiles_m, tn = n_fastest ? t % tiles_n : t / tiles_m;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = blockIdx.y * ksplit_len;
  const int kend = min(K, kbeg + ksplit_len);
  C += (int64_t)blockIdx.y * split_stride;

  const LanePos lp = lane_pos<Cfg>();
  const bool second_group = KW > 1 && (int)(threadIdx.x >> 6) >= Cfg::G;
  AuxRegs<Cfg, EPI> ar;
  if (!second_group) epi_prefetch_aux<Cfg, EPI>(ar, aux, ldaux, M, N, m0, n0, lp);

  typename Cfg::Acc accs;
  gemm_mainloop<BM, BN, A_KC, B_KC, false, KW, PD, ST, FINE, DUAL>(accs, A, lda, B, ldb, M, N, kbeg, kend, m0, n0, smem);

  if (second_group) return;  // the second wave group handed its partial sums over in the main loop
  epi_store<Cfg, EPI>(accs, ar, C, ldc, M, N, bias, aux, ldaux, m0, n0, lp, bt.act);
}

// ---- stream-K: the K loops of ALL output tiles as ONE sequence of K-tile iterations, cut into equal pieces --------------
// M = B*L = 3200 tokens gives 400 (N = 512) or 800 (N = 2048) 64x64 tiles on 256 CUs: 1-2 / 3-4 tiles per CU, and the
// launch takes as long as the fullest CU (profiles/r02/gemm_timeline.json: the CUs with one tile are done at 12.8 us,
// those with two at 20 us).  Here `gridDim.x` workers (2 per CU) each take total_iters / workers consecutive iterations
// of the sequence [tile 0: k-tiles 0..nk) [tile 1: ...) ...; a worker's range starts inside a tile, covers whole tiles,
// and ends inside one.  The worker that STARTS a tile owns it: it keeps its accumulators, waits for the partial sums of
// the workers that continued the tile (each of those handles that piece FIRST and publishes it before doing anything
// else, so the wait is short and cannot deadlock: the only thing a worker ever waits for is work a later worker does
// unconditionally at its very start), adds them in worker order and runs the epilogue.  Deterministic: the summation
// order of every output element is fixed by (shape, worker count).
// Partials cross XCDs (private, mutually incoherent L2s): they are written and read with sc0 sc1 (system-coherent)
// buffer accesses, and the flag is an agent-scope atomic set after the stores were acknowledged (s_waitcnt vmcnt(0)).
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int SK_MAX_WORKERS = 1024;
constexpr int SK_PART_FLOATS = 64 * 64;                   // one 64x64 tile of partial sums per worker
constexpr int SK_COHERENT = (1 << 4) | 1;                 // gfx940+ buffer cache policy: sc1 | sc0
constexpr int64_t SK_SCRATCH_BYTES = (int64_t)SK_MAX_WORKERS * SK_PART_FLOATS * 4 + SK_MAX_WORKERS * 4;

template <bool A_KC, bool B_KC, int EPI>
__global__ void __launch_bounds__(GEMM_THREADS)
gemm_sk_kernel(const float* __restrict__ A, int64_t lda, const float* __restrict__ B, int64_t ldb,
               float* __restrict__ C, int64_t ldc, int M, int N, int K, const float* __restrict__ bias,
               float* __restrict__ aux, int64_t ldaux, int tiles_m, int tiles_n, int n_fastest, int act,
               float* __restrict__ part, unsigned* __restrict__ flags, unsigned* __restrict__ status) {
  using Cfg = GemmCfg<64, 64, A_KC, B_KC>;
  __shared__ __attribute__((aligned(16))) float smem[2 * Cfg::STAGE];
  const int nk = (K + GEMM_BK - 1) / GEMM_BK;
  const int64_t total = (int64_t)tiles_m * tiles_n * nk;
  const int G = gridDim.x;
  const int w = xcd_remap(blockIdx.x, G);     // neighbouring workers (which share tiles) sit on the same XCD
  int64_t it = total * w / G;
  const int64_t it_end = total * (w + 1) / G;
  const LanePos lp = lane_pos<Cfg>();
  const int tid = threadIdx.x;
  const bufrsrc rs_part = make_rsrc(part, (int64_t)SK_MAX_WORKERS * SK_PART_FLOATS * 4);

  while (it < it_end) {     // block-uniform
    const int tile = (int)(it / nk);
    const int kf = (int)(it - (int64_t)tile * nk);
    const int kl = (int)min((int64_t)nk, kf + (it_end - it));
    const int tm = n_fastest ? tile / tiles_n : tile % tiles_m, tn = n_fastest ? tile % tiles_n : tile / tiles_m;
    const int m0 = tm * 64, n0 = tn * 64;
    const bool owner = (kf == 0);
    AuxRegs<Cfg, EPI> ar;
    if (owner) epi_prefetch_aux<Cfg, EPI>(ar, aux, ldaux, M, N, m0, n0, lp);
    typename Cfg::Acc accs;
    gemm_mainloop<64, 64, A_KC, B_KC, false, 1, 2, 2>(accs, A, lda, B, ldb, M, N, kf * GEMM_BK, min(K, kl * GEMM_BK), m0, n0, smem);
    auto& acc = accs.v[0][0];
    if (!owner) {
      // publish: [worker][4 x float4][thread]
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        u32x4 v;
        v[0] = __float_as_uint(acc[4 * q]); v[1] = __float_as_uint(acc[4 * q + 1]);
        v[2] = __float_as_uint(acc[4 * q + 2]); v[3] = __float_as_uint(acc[4 * q + 3]);
        __builtin_amdgcn_raw_buffer_store_b128(v, rs_part, (unsigned)(((w * 4 + q) * GEMM_THREADS + tid) * 16), 0, SK_COHERENT);
      }
      __builtin_amdgcn_s_waitcnt(0);          // every lane's stores acknowledged at the coherence point
      __syncthreads();
      if (tid == 0) __hip_atomic_store(&flags[w], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      int covered = kl;
      int u = w + 1;
      while (covered < nk) {                   // block-uniform: the workers that continued this tile, in order
        const int64_t u0 = total * u / G, u1 = total * (u + 1) / G;
        if (tid == 0) {
          unsigned spins = 0;
          while (__hip_atomic_load(&flags[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
            __builtin_amdgcn_s_sleep(4);
            if (++spins > (1u << 22)) {        // ~seconds: never in a healthy launch; flag it instead of hanging the GPU
              if (status) atomicOr(status, (unsigned)PXR_STATUS_GEMM_TIMEOUT);
              break;
            }
          }
          __hip_atomic_store(&flags[u], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // clean for the next launch
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const auto raw = __builtin_amdgcn_raw_buffer_load_b128(rs_part, (unsigned)(((u * 4 + q) * GEMM_THREADS + tid) * 16), 0, SK_COHERENT);
          acc[4 * q + 0] += __uint_as_float(raw[0]);
          acc[4 * q + 1] += __uint_as_float(raw[1]);
          acc[4 * q + 2] += __uint_as_float(raw[2]);
          acc[4 * q + 3] += __uint_as_float(raw[3]);
        }
        covered += (int)min((int64_t)(nk - covered), u1 - u0);
        ++u;
      }
      epi_store<Cfg, EPI>(accs, ar, C, ldc, M, N, bias, aux, ldaux, m0, n0, lp, act);
    }
    it += kl - kf;
    __syncthreads();     // the staging LDS is reused by the next piece
  }
}

// out[i] = sum_z part[z * stride + i]   (fixed order => deterministic)
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const float4* __restrict__ part, float4* __restrict__ out,
                                                            int64_t n4, int64_t stride4, int splits) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  float4 s = part[i];
  for (int z = 1; z < splits; ++z) {
    const float4 v = part[(int64_t)z * stride4 + i];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  out[i] = s;
}

// Column sums, stage 1: part[chunk][n] = sum over the rows of this chunk of x[row][n]
__global__ void __launch_bounds__(256) colsum_partial_kernel(const float* __restrict__ x, int64_t ldx, int M, int N,
                                                             int rows_per_chunk, float* __restrict__ part) {
  __shared__ float red[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + tx;
  const int r0 = blockIdx.y * rows_per_chunk;
  const int r1 = min(M, r0 + rows_per_chunk);
  float s = 0.f;
  if (col < N)
    for (int row = r0 + ty; row < r1; row += 4) s += x[(int64_t)row * ldx + col];
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && col < N) part[(int64_t)blockIdx.y * N + col] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
}
// ---- grouped weight-gradient GEMM ------------------------------------------------------------------------------
// All dW[N,K] = dY[M,N]^T X[M,K] (+ db[N] = column sums of dY) of a backward pass in ONE launch.  Every problem has
// the long token reduction (M = B*L) as its K loop, so with all problems' 64x64 output tiles in one grid (1024 tiles
// for the two SASRec layers at D=512) the chip is full without split-K: no partial buffers, no reduce launches, no
// separate bias-gradient reductions.  Deterministic: each output element is one fixed-order MFMA chain.
__global__ void __launch_bounds__(GEMM_THREADS) grouped_dw_kernel(DwGroup g) {
  using Cfg = GemmCfg<64, 64, false, false>;
  __shared__ __attribute__((aligned(16))) float smem[2 * Cfg::STAGE];
  const int t = xcd_remap(blockIdx.x, g.total_tiles);
  int pi = 0;
#pragma unroll 1
  for (int i = 1; i < g.n; ++i)
    if (t >= g.p[i].tile_begin) pi = i;
  const DwProblem& P = g.p[pi];
  const int local = t - P.tile_begin;
  const int tm = local % P.tiles_m, tn = local / P.tiles_m;
  const int m0 = tm * 64, n0 = tn * 64;
  typename Cfg::Acc accs;
  float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);
  const bool do_bias = (P.db != nullptr) && (tn == 0);
  if (do_bias)
    gemm_mainloop<64, 64, false, false, true>(accs, P.dy, P.N, P.x, P.K, P.N, P.K, 0, P.M, m0, n0, smem, &cs);
  else
    gemm_mainloop<64, 64, false, false, false>(accs, P.dy, P.N, P.x, P.K, P.N, P.K, 0, P.M, m0, n0, smem);
  auto& acc = accs.v;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1, h = lane >> 5, r = lane & 31;
  const int col = n0 + wn * 32 + r;
  if (col < P.K) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = m0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (row < P.N) P.dW[(int64_t)row * P.K + col] = acc[0][0][e];
    }
  }
  if (do_bias) {
    // thread tid staged columns 4*(tid%16) .. +3 of this 64-column block for its k rows: reduce the 16 threads of
    // each column group in fixed order (the main loop ended with a barrier, smem is free)
    float4* red = reinterpret_cast<float4*>(smem);
    red[threadIdx.x] = cs;
    __syncthreads();
    if (threadIdx.x < 16) {
      float4 s = red[threadIdx.x];
      for (int j = 1; j < 16; ++j) {
        const float4 v = red[threadIdx.x + 16 * j];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      }
      const int c = m0 + threadIdx.x * 4;
      if (c + 0 < P.N) P.db[c + 0] = s.x;
      if (c + 1 < P.N) P.db[c + 1] = s.y;
      if (c + 2 < P.N) P.db[c + 2] = s.z;
      if (c + 3 < P.N) P.db[c + 3] = s.w;
    }
  }
}

// batch descriptor of the call in progress on this host thread (set by pxr_gemm_batched_f32; {0} / 1 otherwise)
static thread_local GemmBatch g_bt = GemmBatch{};
static thread_local int g_batch = 1;

template <int BM, int BN, bool A_KC, bool B_KC, int EPI, int KW = 1, int PD = 1, int ST = 2, int FINE = 0, bool DUAL = false>
static int launch_gemm(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M,
                       int N, int K, const float* bias, float* aux, int64_t ldaux, int splits, int ksplit_len,
                       int64_t split_stride, hipStream_t st) {
  const GemmBatch bt = g_bt;
  const int batch = g_batch;
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  static const int xcd_env = getenv("PXR_GEMM_XCD") ? atoi(getenv("PXR_GEMM_XCD")) : -1;   // A/B knob: 0 = m fastest, 1 = n
  const int n_fastest = xcd_env >= 0 ? xcd_env : (M > N ? 1 : 0);
  hipLaunchKernelGGL((gemm_kernel<BM, BN, A_KC, B_KC, EPI, KW, PD, ST, FINE, DUAL>), dim3(tiles_m * tiles_n, splits, batch),
                     dim3(GemmCfg<BM, BN, A_KC, B_KC, KW, FINE>::NT), 0, st, A, lda, B, ldb, C, ldc, M, N, K, bias, aux, ldaux, tiles_m,
                     tiles_n, ksplit_len, split_stride, n_fastest, bt);
  return pxr_check_launch("pxr_gemm_f32");
}

template <bool A_KC, bool B_KC, int EPI>
static int dispatch_tile(int tile, const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                         int M, int N, int K, const float* bias, float* aux, int64_t ldaux, int splits,
                         int ksplit_len, int64_t split_stride, hipStream_t st) {
  static const int pd = getenv("PXR_GEMM_PD") ? atoi(getenv("PXR_GEMM_PD")) : 2;   // prefetch depth (tuning knob)
  static const int st1 = getenv("PXR_GEMM_STAGES") ? atoi(getenv("PXR_GEMM_STAGES")) == 1 : 0;   // single LDS buffer
#define PXR_TILE_PD(BM_, BN_, KW_, PD_)                                                                              \
  do {                                                                                                               \
    if (st1)                                                                                                         \
      return launch_gemm<BM_, BN_, A_KC, B_KC, EPI, KW_, PD_, 1>(A, lda, B, ldb, C, ldc, M, N, K, bias, aux, ldaux,  \
                                                                 splits, ksplit_len, split_stride, st);             \
    return launch_gemm<BM_, BN_, A_KC, B_KC, EPI, KW_, PD_, 2>(A, lda, B, ldb, C, ldc, M, N, K, bias, aux, ldaux,    \
                                                               splits, ksplit_len, split_stride, st);               \
  } while (0)
#define PXR_TILE(BM_, BN_, KW_)                  \
  do {                                           \
    if (pd == 1) PXR_TILE_PD(BM_, BN_, KW_, 1);  \
    PXR_TILE_PD(BM_, BN_, KW_, 2);               \
  } while (0)
  switch (tile) {
    case 128: PXR_TILE_PD(128, 128, 1, 1);   // 1.7 us of MFMA work per K tile: one tile of prefetch is enough
    case 12864: PXR_TILE(128, 64, 1);
    case 64128: PXR_TILE(64, 128, 1);
    case 642:  // 64x64 tile, 8 waves: two wave groups split the k-steps (see GemmCfg KW)
      PXR_TILE(64, 64, 2);
    case 3264:  // 32x64 tile, 4 waves = 1x2 wave grid x 2 k-groups: twice as many (independent) workgroups
      PXR_TILE(32, 64, 2);
    case 1281:   // 128x128 tile cut into 16 wave tiles of 32x32 (1024 threads): half the L2 -> LDS traffic of 64x64
      return launch_gemm<128, 128, A_KC, B_KC, EPI, 1, 2, 2, 1>(A, lda, B, ldb, C, ldc, M, N, K, bias, aux, ldaux, splits,
                                                                ksplit_len, split_stride, st);
    case 1282:   // 128x128 tile, 8 wave tiles of 64x32 (512 threads)
      return launch_gemm<128, 128, A_KC, B_KC, EPI, 1, 2, 2, 2>(A, lda, B, ldb, C, ldc, M, N, K, bias, aux, ldaux, splits,
                                                                ksplit_len, split_stride, st);
    case 641:    // 64x64 tile, 4 wave tiles of 32x32, two accumulator chains per wave (even / odd k sub-steps)
      return launch_gemm<64, 64, A_KC, B_KC, EPI, 1, 2, 2, 0, true>(A, lda, B, ldb, C, ldc, M, N, K, bias, aux, ldaux, splits,
                                                                     ksplit_len, split_stride, st);
    case 128611:  // 128x64 tile, 8 wave tiles of 32x32, two accumulator chains per wave
      return launch_gemm<128, 64, A_KC, B_KC, EPI, 1, 2, 2, 1, true>(A, lda, B, ldb, C, ldc, M, N, K, bias, aux, ldaux, splits,
                                                                      ksplit_len, split_stride, st);
    case 12861:  // 128x64 tile, 8 wave tiles of 32x32 (512 threads)
      return launch_gemm<128, 64, A_KC, B_KC, EPI, 1, 2, 2, 1>(A, lda, B, ldb, C, ldc, M, N, K, bias, aux, ldaux, splits,
                                                               ksplit_len, split_stride, st);
    default: PXR_TILE(64, 64, 1);
  }
#undef PXR_TILE_PD
#undef PXR_TILE
}


// Scratch of the stream-K kernel (partials + flags): two stream-K launches may only run concurrently if they do not
// share it, so every stream that launches one gets its own block out of a small pool.  The pool is allocated and zeroed
// on the first use -- which must not happen inside a stream capture (every capture in this package is preceded by eager
// warm-up steps); handing a pool block to a new stream (e.g. the capture stream of a hipGraph) allocates nothing.
struct SkScratch { float* part; unsigned* flags; };
constexpr int SK_POOL = 8;
static std::mutex g_sk_mu;
static char* g_sk_pool = nullptr;
static int g_sk_used = 0;
static std::unordered_map<hipStream_t, int> g_sk_block;
static int sk_scratch_for(hipStream_t st, SkScratch* out) {
  std::lock_guard<std::mutex> lk(g_sk_mu);
  if (!g_sk_pool) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
      pxr_set_error("pxr_gemm_f32: the first stream-K GEMM of the process happens inside a stream capture; run one eager "
                    "step first (or PXR_GEMM_SK=0)");
      return PXR_ERR_WORKSPACE;
    }
    void* p = nullptr;
    if (hipMalloc(&p, SK_SCRATCH_BYTES * SK_POOL) != hipSuccess || hipMemset(p, 0, SK_SCRATCH_BYTES * SK_POOL) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {
      pxr_set_error("pxr_gemm_f32: cannot allocate the stream-K scratch pool (%lld bytes): %s",
                    (long long)(SK_SCRATCH_BYTES * SK_POOL), hipGetErrorString(hipGetLastError()));
      return PXR_ERR_WORKSPACE;
    }
    g_sk_pool = (char*)p;
  }
  auto f = g_sk_block.find(st);
  int blk;
  if (f != g_sk_block.end()) blk = f->second;
  else {
    if (g_sk_used >= SK_POOL) {
      pxr_set_error("pxr_gemm_f32: more than %d streams launch stream-K GEMMs (PXR_GEMM_SK=0 turns them off)", SK_POOL);
      return PXR_ERR_WORKSPACE;
    }
    blk = g_sk_used++;
    g_sk_block[st] = blk;
  }
  char* base = g_sk_pool + (int64_t)blk * SK_SCRATCH_BYTES;
  *out = SkScratch{(float*)base, (unsigned*)(base + (int64_t)SK_MAX_WORKERS * SK_PART_FLOATS * 4)};
  return PXR_OK;
}

// After a PXR_STATUS_GEMM_TIMEOUT (a worker gave up waiting for a flag) the flag words are in an unknown state -- the late
// publisher may still raise a flag nobody lowers, and the NEXT launch's consumers would then read an unpublished partial without
// waiting (advisor r4).  The host calls this when it sees the status bit: waits for the device, then zeroes every block's flags.
extern "C" int pxr_gemm_reset_flags(void) {
  std::lock_guard<std::mutex> lk(g_sk_mu);
  if (!g_sk_pool) return PXR_OK;
  if (hipDeviceSynchronize() != hipSuccess) { pxr_set_error("pxr_gemm_reset_flags: device synchronisation failed"); return PXR_ERR_LAUNCH; }
  for (int blk = 0; blk < g_sk_used; ++blk) {
    char* base = g_sk_pool + (int64_t)blk * SK_SCRATCH_BYTES;
    if (hipMemset(base + (int64_t)SK_MAX_WORKERS * SK_PART_FLOATS * 4, 0, (size_t)SK_MAX_WORKERS * 4) != hipSuccess) {
      pxr_set_error("pxr_gemm_reset_flags: memset failed");
      return PXR_ERR_LAUNCH;
    }
  }
  return hipDeviceSynchronize() == hipSuccess ? PXR_OK : PXR_ERR_LAUNCH;
}

// the flag block of a stream (SK_MAX_WORKERS zero-initialised words that every user leaves zeroed): shared with the split-K weight
// gradient launch of gemm_p3.hip, which runs on the same stream as any stream-K GEMM that could use it (never concurrently)
int pxr_stream_flags(hipStream_t st, unsigned** flags, int* n_flags) {
  SkScratch sc{};
  const int rc = sk_scratch_for(st, &sc);
  if (rc != PXR_OK) return rc;
  *flags = sc.flags;
  *n_flags = SK_MAX_WORKERS;
  return PXR_OK;
}

// Where stream-K pays (tools/sk_sweep.py, M = 3200 tokens, us per launch, tile-per-workgroup -> stream-K with 768 workers):
//   N=512 K=1536 (dX of the QKV projection) 58.0 -> 52.9;  N=512 K=1024 40.7 -> 38.5 / 37.3 -> 38.8;
//   N=512 K=512 21.3 -> 24.9;  N=1024 K=512 45.6 -> 48.3;  N=1536 K=512 46.3 -> 51.8.
// Publishing and fetching a partial tile through coherent memory costs ~3-4 us per launch, more than the 22 % idle
// tail of a 400-tile launch is worth unless the K loop is long: the heuristic takes it for one to two tiles per CU
// and K >= 1536 only.
static int sk_workers(int64_t tiles, int nk, int batch, int splits, int forced_workers) {
  static const int mode = getenv("PXR_GEMM_SK") ? atoi(getenv("PXR_GEMM_SK")) : 1;      // 0 off, 1 heuristic, 2 always
  static const int wg_env = getenv("PXR_GEMM_SK_WGS") ? atoi(getenv("PXR_GEMM_SK_WGS")) : 768;
  const int wg = forced_workers > 0 ? forced_workers : wg_env;
  if (batch != 1 || splits != 1 || nk < 4) return 0;
  if (forced_workers == 0 && mode == 0) return 0;
  if (forced_workers == 0 && mode == 1) {
    if (tiles <= 256 || tiles > 512 || nk < 48) return 0;
  }
  int64_t g = wg < 16 ? 16 : (wg > SK_MAX_WORKERS ? SK_MAX_WORKERS : wg);
  const int64_t total = tiles * nk;
  if (g > total / 4) g = total / 4;       // at least 4 K tiles per worker
  return g < 1 ? 0 : (int)g;
}

template <bool A_KC, bool B_KC, int EPI>
static int launch_gemm_sk(int workers, const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M,
                          int N, int K, const float* bias, float* aux, int64_t ldaux, hipStream_t st) {
  SkScratch sc;
  const int rc = sk_scratch_for(st, &sc);
  if (rc != PXR_OK) return rc;
  const int tiles_m = (M + 63) / 64, tiles_n = (N + 63) / 64;
  static const int xcd_env = getenv("PXR_GEMM_XCD") ? atoi(getenv("PXR_GEMM_XCD")) : -1;
  const int n_fastest = xcd_env >= 0 ? xcd_env : (M > N ? 1 : 0);
  hipLaunchKernelGGL((gemm_sk_kernel<A_KC, B_KC, EPI>), dim3(workers), dim3(GEMM_THREADS), 0, st, A, lda, B, ldb, C, ldc, M, N, K,
                     bias, aux, ldaux, tiles_m, tiles_n, n_fastest, g_bt.act, sc.part, sc.flags, (unsigned*)pxr_status_word());
  return pxr_check_launch("pxr_gemm_f32(stream-K)");
}

}  // namespace pxr

using namespace pxr;

// GEMM mode of the process: "bf16x3" (default) = exact 3 x bf16 operand split on the bf16 matrix pipe (gemm_b3.cuh),
// "f32" = the f32-input MFMA kernels.  PXR_GEMM_MODE, or pxr_set_gemm_mode (tests, A/B runs).
static int g_gemm_mode = -1;
static bool gemm_mode_b3() {
  if (g_gemm_mode < 0) {
    const char* e = getenv("PXR_GEMM_MODE");
    g_gemm_mode = (e && (e[0] == 'f' || e[0] == 'F')) ? 0 : 1;
  }
  return g_gemm_mode == 1;
}
extern "C" int pxr_set_gemm_mode(int bf16x3) {
  g_gemm_mode = bf16x3 ? 1 : 0;
  return PXR_OK;
}
extern "C" int pxr_get_gemm_mode(void) { return gemm_mode_b3() ? 1 : 0; }

// Bytes of workspace pxr_gemm_f32 may use for split-K partials (0 => never splits).
extern "C" int64_t pxr_gemm_ws_bytes(int a_kc, int b_kc, int M, int N, int K) {
  (void)a_kc; (void)b_kc; (void)K;
  return (int64_t)16 * M * N * (int64_t)sizeof(float);  // at most 16 splits
}

// General entry: C[M,N] = A_op * B_op with the storage flavours of gemm_f32.cuh.
//   tile_hint: 0 = heuristic, 64 / 128 = force that square tile.   split_hint: 0 = heuristic, >=1 = force.
extern "C" int pxr_gemm_f32(int a_kc, int b_kc, int M, int N, int K, const float* A, int64_t lda, const float* B,
                            int64_t ldb, float* C, int64_t ldc, int epilogue, const float* bias, float* aux,
                            int64_t ldaux, void* ws, int64_t ws_bytes, int tile_hint, int split_hint,
                            void* stream) {
  PXR_REQUIRE(A && B && C, "pxr_gemm_f32: null operand");
  PXR_REQUIRE(M >= 0 && N >= 0 && K >= 0, "pxr_gemm_f32: negative dim");
  if (M == 0 || N == 0) return PXR_OK;
  PXR_REQUIRE((lda % 4) == 0 && (ldb % 4) == 0, "pxr_gemm_f32: leading dims must be multiples of 4 floats");
  PXR_REQUIRE((((uintptr_t)A | (uintptr_t)B) & 15) == 0, "pxr_gemm_f32: operands must be 16-byte aligned");
  // the contiguous extent of each operand is read as float4: a multiple of 4, or rows padded to one (ld >= extent rounded
  // up; the caller keeps the pad FINITE -- zero when it lies inside the reduction -- e.g. attention scores [T, ld])
  const int ext_a = a_kc ? K : M, ext_b = b_kc ? K : N;
  PXR_REQUIRE(ext_a % 4 == 0 || lda >= ((ext_a + 3) & ~3), "pxr_gemm_f32: A contiguous extent must be a multiple of 4 (or padded)");
  PXR_REQUIRE(ext_b % 4 == 0 || ldb >= ((ext_b + 3) & ~3), "pxr_gemm_f32: B contiguous extent must be a multiple of 4 (or padded)");
  PXR_REQUIRE(epilogue >= 0 && epilogue <= EPI_LAST, "pxr_gemm_f32: bad epilogue %d", epilogue);
  if (!epi_operands_ok("pxr_gemm_f32", epilogue, bias, aux)) return PXR_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;

  const int64_t t128 = (int64_t)((M + 127) / 128) * ((N + 127) / 128);
  bool big = (t128 >= 384);  // >= 1.5 waves of 128x128 tiles over 256 CUs; otherwise 64x64 tiles fill the chip better
  // big problems: the 128x128 tile cut into 16 wave tiles of 32x32 (1024 threads, 8 waves per SIMD at 2 workgroups
  // per CU) beats 4 waves of 64x64 by 7-20 % (tools/big_gemm_tiles.py: scoring GEMM 120 -> 133 TFLOP/s)
  static const int big_tile = getenv("PXR_GEMM_BIG_TILE") ? atoi(getenv("PXR_GEMM_BIG_TILE")) : 1281;
  int tile = big ? big_tile : 64;
  // 192..256 tiles of 128x128 = one 16-wave workgroup on (almost) every CU in a single round: +3..9 % over 64x64 at
  // a dozen shapes, while 150/175/304 tiles lose 13-28 % (tools/tile_rule_check.py)
  if (!big && t128 >= 192 && t128 <= 256) tile = 1281;
  static const int small_tile = getenv("PXR_GEMM_SMALL_TILE") ? atoi(getenv("PXR_GEMM_SMALL_TILE")) : 64;
  if (tile == 64) tile = small_tile;
  if (tile_hint == 641 || tile_hint == 128611 || tile_hint == 128 || tile_hint == 64 || tile_hint == 12864 || tile_hint == 64128 || tile_hint == 642 || tile_hint == 3264 || tile_hint == 1281 || tile_hint == 12861 || tile_hint == 1282) tile = tile_hint;
  const int b3_hint = (tile_hint == 9064 || tile_hint == 91281) ? tile_hint : 0;
  if (b3_hint) tile = b3_hint == 9064 ? 64 : 1281;
  // tile_hint 6464: force the stream-K kernel (64x64 tiles) with split_hint workers (0 = default) -- tests and sweeps
  const int sk_force = tile_hint == 6464 ? (split_hint > 0 ? split_hint : 768) : 0;
  if (sk_force) { tile = 64; split_hint = 1; }
  const int64_t t64 = (int64_t)((M + 63) / 64) * ((N + 63) / 64);
  const int bm = (tile == 128 || tile == 12864 || tile == 1281 || tile == 12861 || tile == 128611 || tile == 1282) ? 128 : (tile == 3264 ? 32 : 64);
  const int bn = (tile == 128 || tile == 64128 || tile == 1281 || tile == 1282) ? 128 : 64;
  const int64_t tiles = (int64_t)((M + bm - 1) / bm) * ((N + bn - 1) / bn);
  PXR_REQUIRE(tiles < (1ll << 31), "pxr_gemm_f32: too many tiles");

  // split-K only for the plain epilogue (weight gradients: few output tiles, long token reduction)
  int splits = 1;
  const int nk = (K + GEMM_BK - 1) / GEMM_BK;
  if (epilogue == EPI_NONE && ws && g_batch == 1) {
    if (split_hint >= 1) splits = split_hint;
    else if (tiles < 256 && nk >= 16) {
      splits = (int)((512 + tiles - 1) / tiles);
      if (splits > nk / 4) splits = nk / 4;
    }
    if (splits > 16) splits = 16;
    if (splits < 1) splits = 1;
    while (splits > 1 && (int64_t)splits * M * N * 4 > ws_bytes) --splits;
  }
  int ktiles_per = (nk + splits - 1) / splits;
  if (ktiles_per < 1) ktiles_per = 1;
  splits = (nk + ktiles_per - 1) / ktiles_per;
  if (splits < 1) splits = 1;
  const int ksplit_len = (splits == 1) ? (K > 0 ? K : 1) : ktiles_per * GEMM_BK;

  float* Cw = C;
  int64_t ldcw = ldc, split_stride = 0;
  if (splits > 1) {
    Cw = (float*)ws;
    ldcw = N;
    split_stride = (int64_t)M * N;
    PXR_REQUIRE((N % 4) == 0 && ldc == N, "pxr_gemm_f32: split-K needs a dense C with N %% 4 == 0");
  }

  int rc;
  // bf16x3 mode (default): the heuristic's choices run on the bf16 matrix pipe (gemm_b3.cuh); an explicit f32 tile_hint
  // keeps the f32-input MFMA kernel (tests / sweeps), 9064 / 91281 force the bf16x3 64x64 / 128x128 tile.
  const bool b3 = b3_hint ? true : (gemm_mode_b3() && tile_hint == 0);
  if (b3) {
    const int t3 = b3_hint == 91281 ? 1281 : (b3_hint == 9064 ? 64 : ((t128 >= 384 || (t128 >= 192 && t128 <= 256)) ? 1281 : 64));
    rc = gemm_b3_launch(a_kc, b_kc, epilogue, t3, A, lda, B, ldb, Cw, ldcw, M, N, K, bias, aux, ldaux, splits, ksplit_len,
                        split_stride, g_bt, g_batch, st);
    if (rc != PXR_OK) return rc;
    if (splits > 1) {
      const int64_t n4 = (int64_t)M * N / 4;
      hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st,
                         (const float4*)ws, (float4*)C, n4, n4, splits);
      return pxr_check_launch("pxr_gemm_f32(split-K reduce)");
    }
    return PXR_OK;
  }
  int skw = sk_force ? sk_workers(tiles, nk, g_batch, 1, sk_force)
                     : ((tile_hint == 0 && split_hint == 0) ? sk_workers(t64, nk, g_batch, splits, 0) : 0);
  if (skw > 0 && !sk_force) {
    // the heuristic's choice needs a scratch block for this stream: when the pool is exhausted (a long-lived process that
    // keeps taking fresh streams) or cannot be created here (inside a capture), take the tile-per-workgroup kernel instead
    SkScratch probe;
    if (sk_scratch_for(st, &probe) != PXR_OK) skw = 0;
  }
#define PXR_GEMM_CASE(AK, BK_, E)                                                                            \
  rc = skw > 0 ? launch_gemm_sk<AK, BK_, E>(skw, A, lda, B, ldb, C, ldc, M, N, K, bias, aux, ldaux, st)        \
               : dispatch_tile<AK, BK_, E>(tile, A, lda, B, ldb, Cw, ldcw, M, N, K, bias, aux, ldaux, splits, ksplit_len, \
                                           split_stride, st)
#define PXR_GEMM_FWD(E) case E: PXR_GEMM_CASE(true, true, E); break;
#define PXR_GEMM_BWD(E) case E: PXR_GEMM_CASE(true, false, E); break;
  if (a_kc && b_kc) {
    switch (epilogue) {
      PXR_EPI_FWD(PXR_GEMM_FWD)
      default: pxr_set_error("pxr_gemm_f32: epilogue %d unsupported for (KC,KC)", epilogue); return PXR_ERR_BAD_ARG;
    }
  } else if (a_kc && !b_kc) {
    switch (epilogue) {
      PXR_EPI_BWD_F32(PXR_GEMM_BWD)
      default: pxr_set_error("pxr_gemm_f32: epilogue %d unsupported for (KC,XC)", epilogue); return PXR_ERR_BAD_ARG;
    }
  } else if (!a_kc && !b_kc) {
    PXR_REQUIRE(epilogue == EPI_NONE, "pxr_gemm_f32: epilogue %d unsupported for (XC,XC)", epilogue);
    PXR_GEMM_CASE(false, false, EPI_NONE);
  } else {
    pxr_set_error("pxr_gemm_f32: (XC,KC) operand combination is not instantiated");
    return PXR_ERR_BAD_ARG;
  }
#undef PXR_GEMM_FWD
#undef PXR_GEMM_BWD
#undef PXR_GEMM_CASE
  if (rc != PXR_OK) return rc;

  if (splits > 1) {
    const int64_t n4 = (int64_t)M * N / 4;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st,
                       (const float4*)ws, (float4*)C, n4, n4, splits);
    return pxr_check_launch("pxr_gemm_f32(split-K reduce)");
  }
  return PXR_OK;
}

// `batch` independent problems of one shape in ONE launch (grid.z): operand z lives at base + (z / nb2) * s1 +
// (z % nb2) * s2 floats (two-level strides: e.g. image n and head h of a packed [n, T, 3*heads*d] projection).  No
// split-K, no workspace; epilogues as pxr_gemm_f32 (bias / aux are shared by all problems).  Used by the attention of
// the ViT image encoder (S = Q K^T, O = P V and their backward contractions; model/vit_native.py).
extern "C" int pxr_gemm_batched_f32(int a_kc, int b_kc, int M, int N, int K, const float* A, int64_t lda, const float* B,
                                    int64_t ldb, float* C, int64_t ldc, int batch, int nb2, int64_t a1, int64_t a2,
                                    int64_t b1, int64_t b2, int64_t c1, int64_t c2, int tile_hint, void* stream) {
  PXR_REQUIRE(batch >= 1 && nb2 >= 1, "pxr_gemm_batched_f32: bad batch %d / nb2 %d", batch, nb2);
  PXR_REQUIRE(((a1 | a2 | b1 | b2) & 3) == 0, "pxr_gemm_batched_f32: operand strides must be multiples of 4 floats");
  int rc = PXR_OK;
  for (int z0 = 0; z0 < batch && rc == PXR_OK; z0 += 65535 / nb2 * nb2) {   // grid.z <= 65535: whole groups per launch
    const int nz = min(batch - z0, 65535 / nb2 * nb2);
    const int64_t g0 = z0 / nb2;
    g_bt = GemmBatch{nb2, a1, a2, b1, b2, c1, c2, 0};
    g_batch = nz;
    rc = pxr_gemm_f32(a_kc, b_kc, M, N, K, A + g0 * a1, lda, B + g0 * b1, ldb, C + g0 * c1, ldc, EPI_NONE, nullptr, nullptr,
                      0, nullptr, 0, tile_hint ? tile_hint : (gemm_mode_b3() ? 9064 : 64), 1, stream);
    g_bt = GemmBatch{};
    g_batch = 1;
  }
  return rc;
}

// y[M,N] = x[M,K] W[N,K]^T + b   (act: 0 none, 1 erf-GELU with the pre-activation saved to `pre`, 2 erf-GELU with
// gelu'(pre-activation) saved to `pre` instead -- the form the training step uses: the backward is one multiply)
extern "C" int pxr_linear_fwd_f32(const float* x, const float* W, const float* b, float* y, float* pre, int M,
                                  int N, int K, int act, void* stream) {
  PXR_REQUIRE(act >= 0 && act <= ACT_SELU, "pxr_linear_fwd_f32: bad act %d", act);
  if (act >= ACT_RELU) {   // relu / swish / tanh / sigmoid / selu: act'(pre-activation) saved to `pre`
    g_bt = GemmBatch{};
    g_bt.act = act;
    const int rc = pxr_gemm_f32(1, 1, M, N, K, x, K, W, K, y, N, EPI_BIAS_ACT_GRAD, b, pre, N, nullptr, 0, 0, 0, stream);
    g_bt = GemmBatch{};
    return rc;
  }
  const int epi = act == 2 ? EPI_BIAS_GELU_GRAD : (act == 1 ? EPI_BIAS_GELU : (b ? EPI_BIAS : EPI_NONE));
  return pxr_gemm_f32(1, 1, M, N, K, x, K, W, K, y, N, epi, b, pre, N, nullptr, 0, 0, 0, stream);
}
// dx[M,K] = dy[M,N] W[N,K]     dgelu_pre != NULL: dx *= gelu'(dgelu_pre) (through the FFN activation, from the saved
//                              pre-activation);  mul != NULL: dx *= mul (gelu' saved by act = 2);
//                              add != NULL: dx += add (the residual branch's gradient).  At most one of the three.
extern "C" int pxr_linear_bwd_input_f32(const float* dy, const float* W, float* dx, const float* dgelu_pre,
                                        const float* add, const float* mul, int M, int N, int K, void* stream) {
  PXR_REQUIRE((dgelu_pre != nullptr) + (add != nullptr) + (mul != nullptr) <= 1,
              "pxr_linear_bwd_input_f32: dgelu_pre, add and mul are mutually exclusive");
  const float* aux = dgelu_pre ? dgelu_pre : (add ? add : mul);
  const int epi = dgelu_pre ? EPI_MUL_DGELU : (add ? EPI_ADD : (mul ? EPI_MUL : EPI_NONE));
  return pxr_gemm_f32(1, 0, M, K, N, dy, N, W, K, dx, K, epi, nullptr, const_cast<float*>(aux), K, nullptr, 0, 0, 0,
                      stream);
}
// dW[N,K] = dy[M,N]^T x[M,K]   (reduction over the M tokens, split-K through ws)
extern "C" int pxr_linear_bwd_weight_f32(const float* dy, const float* x, float* dW, int M, int N, int K, void* ws,
                                         int64_t ws_bytes, void* stream) {
  return pxr_gemm_f32(0, 0, N, K, M, dy, N, x, K, dW, K, EPI_NONE, nullptr, nullptr, 0, ws, ws_bytes, 0, 0, stream);
}

static inline int colsum_rows_per_chunk(int M) {
  int rpc = (M + 127) / 128;  // <= 128 partial rows
  return rpc < 32 ? 32 : rpc;
}
extern "C" int pxr_colsum_partial_rows(int M) {
  const int rpc = colsum_rows_per_chunk(M);
  return (M + rpc - 1) / rpc;
}
extern "C" int64_t pxr_colsum_ws_bytes(int M, int N) {
  const int rpc = colsum_rows_per_chunk(M);
  const int chunks = (M + rpc - 1) / rpc;
  return (int64_t)chunks * N * (int64_t)sizeof(float);
}
// out[n] = sum_m x[m][n]  -- bias gradients (autograd of nn.Linear bias) and the position-embedding
// gradient (sum over the batch of dx0 viewed as [B, L*D]); two fixed-order stages => deterministic.
extern "C" int pxr_colsum_f32(const float* x, int64_t ldx, int M, int N, float* out, void* ws, int64_t ws_bytes,
                              void* stream) {
  PXR_REQUIRE(x && ws, "pxr_colsum_f32: null pointer");
  PXR_REQUIRE(M > 0 && N > 0, "pxr_colsum_f32: empty input");
  const int rows_per_chunk = colsum_rows_per_chunk(M);
  const int chunks = (M + rows_per_chunk - 1) / rows_per_chunk;
  if ((int64_t)chunks * N * 4 > ws_bytes) {
    pxr_set_error("pxr_colsum_f32: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)chunks * N * 4);
    return PXR_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(colsum_partial_kernel, dim3((N + 63) / 64, chunks), dim3(256), 0, st, x, ldx, M, N,
                     rows_per_chunk, (float*)ws);
  int rc = pxr_check_launch("pxr_colsum_f32(partial)");
  if (rc) return rc;
  if (!out) return PXR_OK;  // deferred: ws holds pxr_colsum_partial_rows(M) x N partial sums for a later multi-reduce
  hipLaunchKernelGGL(pxr_reduce_partials_kernel, dim3((N + PXR_RED_CX - 1) / PXR_RED_CX), dim3(256), 0, st, (const float*)ws, chunks, N,
                     out, out, N);
  return pxr_check_launch("pxr_colsum_f32(final)");
}

// Weight AND bias gradients of up to 16 nn.Linear layers in one launch (see grouped_dw_kernel):
//   dW[i] [N_i,K_i] = dy[i] [M_i,N_i]^T x[i] [M_i,K_i];   db[i] [N_i] = column sums of dy[i]   (db[i] may be NULL).
extern "C" int pxr_grouped_linear_bwd_weight_f32(int n, const float* const* dy, const float* const* x,
                                                 float* const* dW, float* const* db, const int* M, const int* N,
                                                 const int* K, void* stream) {
  PXR_REQUIRE(n >= 1 && n <= DW_MAX && dy && x && dW && db && M && N && K,
              "pxr_grouped_linear_bwd_weight_f32: bad args (n=%d, max %d)", n, DW_MAX);
  DwGroup g{};
  g.n = n;
  int tiles = 0;
  for (int i = 0; i < n; ++i) {
    PXR_REQUIRE(dy[i] && x[i] && dW[i] && M[i] > 0 && N[i] > 0 && K[i] > 0 && N[i] % 4 == 0 && K[i] % 4 == 0,
                "pxr_grouped_linear_bwd_weight_f32: problem %d has a bad shape", i);
    PXR_REQUIRE((((uintptr_t)dy[i] | (uintptr_t)x[i]) & 15) == 0, "pxr_grouped_linear_bwd_weight_f32: unaligned operand");
    DwProblem& P = g.p[i];
    P.dy = dy[i]; P.x = x[i]; P.dW = dW[i]; P.db = db[i]; P.M = M[i]; P.N = N[i]; P.K = K[i];
    P.tile_begin = tiles;
    P.tiles_m = (N[i] + 63) / 64;
    tiles += P.tiles_m * ((K[i] + 63) / 64);
  }
  g.total_tiles = tiles;
  if (gemm_mode_b3()) return grouped_dw_b3_launch(g, (hipStream_t)stream);
  hipLaunchKernelGGL(grouped_dw_kernel, dim3(tiles), dim3(GEMM_THREADS), 0, (hipStream_t)stream, g);
  return pxr_check_launch("pxr_grouped_linear_bwd_weight_f32");
}
