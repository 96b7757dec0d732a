// widedeep.hip -- WideDeep (reference code/REC/model/IDNet/widedeep.py): a wide sum of per-item scalars plus an MLP over the
// concatenated embeddings of the L history items and the target.
//
//   y(row)  = sum_w wide[row_w] + wide_bias + predict(mlp(concat_w deep[row_w]))           row = [profile (L) | target]
//   x_b     = y([profile_b | p_b]) - y([profile_b | n_b]);    loss = -mean_b log(1e-8 + sigmoid(x_b))     (widedeep.py:53-63)
//
// The first Linear splits over the concatenation: W1 [h1, (L + 1) D] = [W1h | W1t], z1 = W1h xh + W1t xt + b1.  The two planes of a
// sample share xh, so the library GEMMs make Zh = Xh W1h^T for B rows and Zt = Xt W1t^T for 2 B rows and the join kernel here adds
// them.  In x_b the history's wide terms, wide_bias and the predict bias cancel: x_b = <a_last(+) - a_last(-), w_p> + wide[p_b] -
// wide[n_b], which is what the head computes; their gradients are exact zeros.
// Training side: the join (forward, backward), the head (forward, backward: last-layer gradient, d w_p, the dense wide gradient).
// Rows of every [2 B, *] operand: r = 2 b + c (c = 0 the positive's plane, 1 the negative's).  Every sum has one fixed order; no
// atomics on floats.
//
// Evaluation side (wd_topk_kernel): with T [N, h1] = deep W1t^T + b1 (once per evaluation), h_b = W1h xh_b and s_b = the window's
// wide terms + wide_bias + b_p (once per user),
//   score[b, n] = s_b + wide[n] + <w_p, relu(W2 relu(T[n] + h_b) + b2)>                  (one hidden layer: <w_p, relu(T[n] + h_b)>)
// A workgroup owns one user and a range of 128-item tiles (din_topk_kernel's loop order and LDS plan: the activation tile and W2):
// per tile it adds h_b to the T tile, applies the ReLU into LDS, multiplies the tile with W2 on the fp32-operand MFMA, applies the
// second ReLU, and 128 threads -- one per item -- finish with w_p, the wide terms, the masks (item 0, the ragged edge, the user's
// full history as a bitmap) and a per-thread top-K list; the lists are merged by wave shuffles and pxr_topk_merge.  No [B, N, *]
// value reaches memory.
#include "gemm_f32.cuh"
#include "topk_mlp_tail.cuh"
#include "topk_select.cuh"

namespace pxr {

// ---------------------------------------------------------------------------------------------------- training: the join
// a1[r, j] = relu(zh[r / 2, j] + zt[r, j] + b1[j]),  der[r, j] = [a1 > 0]
__global__ void __launch_bounds__(256) wd_join_kernel(const float* __restrict__ zh, const float* __restrict__ zt,
                                                      const float* __restrict__ b1, int64_t n, int h1, float* __restrict__ a1,
                                                      float* __restrict__ der) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / h1;
    const int j = (int)(e - r * h1);
    const float z = (zh[(r >> 1) * h1 + j] + zt[e]) + b1[j];
    a1[e] = fmaxf(z, 0.f);
    der[e] = z > 0.f ? 1.f : 0.f;
  }
}

// dzh[b, j] = dz1[2 b, j] + dz1[2 b + 1, j]
__global__ void __launch_bounds__(256) wd_join_bwd_kernel(const float* __restrict__ dz1, int64_t n, int h1, float* __restrict__ dzh) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t b = e / h1;
    const int j = (int)(e - b * h1);
    dzh[e] = dz1[(2 * b) * h1 + j] + dz1[(2 * b + 1) * h1 + j];
  }
}

// ---------------------------------------------------------------------------------------------------- training: the head
// one wave per sample: x_b = <a_last(+) - a_last(-), w_p> + wide[p_b] - wide[n_b] -> head[1 + B + b]
__global__ void __launch_bounds__(64) wd_head_fwd_kernel(const float* __restrict__ alast, const float* __restrict__ wp,
                                                         const float* __restrict__ wide, int64_t n_items,
                                                         const int64_t* __restrict__ target, int B, int hl, float* __restrict__ head,
                                                         int32_t* status) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float* ap = alast + (int64_t)(2 * b) * hl;
  const float* an = ap + hl;
  float acc = 0.f;
  for (int j = lane; j < hl; j += 64) acc += (ap[j] - an[j]) * wp[j];
  acc = wave_sum(acc);
  if (lane == 0) {
    // a target id as an index of the wide vector: flagged and clamped when it lies outside [0, n_items)
    const int64_t p = checked_id(target[2 * b], n_items, status, true), q = checked_id(target[2 * b + 1], n_items, status, true);
    head[1 + B + b] = (acc + wide[p]) - wide[q];
  }
}

// one workgroup: loss = -mean log(1e-8 + sigmoid(x)) -> head[0]; coef[b] = d loss / d x_b -> head[1 + b]
__global__ void __launch_bounds__(256) wd_loss_kernel(float* __restrict__ head, int B) {
  __shared__ float red[256];
  float t = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float sg = 1.0f / (1.0f + expf(-head[1 + B + b]));
    t += logf(1e-8f + sg);
    head[1 + b] = -(1.0f / (float)B) * sg * (1.0f - sg) / (1e-8f + sg);
  }
  t = block_sum256(t, red);
  if (threadIdx.x == 0) head[0] = -t / (float)B;
}

// dz[2 b + c, j] = (c ? -g : g) coef_b w_p[j] act'[2 b + c, j]
__global__ void __launch_bounds__(256) wd_head_bwd_kernel(const float* __restrict__ dact, const float* __restrict__ wp,
                                                          const float* __restrict__ head, const float* __restrict__ gsd, float gscale,
                                                          int64_t n, int hl, float* __restrict__ dz) {
  const float g = gscale * gsd[0];
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / hl;
    const int j = (int)(e - r * hl);
    const float gc = ((r & 1) ? -g : g) * head[1 + (r >> 1)];
    dz[e] = gc * wp[j] * dact[e];
  }
}

// thread j < hl: dwp[j] = sum_b g coef_b (a_last[2 b, j] - a_last[2 b + 1, j]) in ascending b; thread hl: the two cancelled biases.
// The loads of eight samples are issued together (their addresses do not depend on the sum); the additions keep their order.
__global__ void __launch_bounds__(64) wd_predict_grad_kernel(const float* __restrict__ alast, const float* __restrict__ head,
                                                             const float* __restrict__ gsd, float gscale, int B, int hl,
                                                             float* __restrict__ dwp, float* __restrict__ dbp,
                                                             float* __restrict__ dwide_bias) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j == hl) { dbp[0] = 0.f; dwide_bias[0] = 0.f; }
  if (j >= hl) return;
  const float g = gscale * gsd[0];
  float acc = 0.f;
  int b = 0;
  for (; b + 8 <= B; b += 8) {
    float c[8], p[8], q[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      c[u] = head[1 + b + u];
      p[u] = alast[(int64_t)(2 * (b + u)) * hl + j];
      q[u] = alast[(int64_t)(2 * (b + u) + 1) * hl + j];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += (g * c[u]) * (p[u] - q[u]);
  }
  for (; b < B; ++b) acc += (g * head[1 + b]) * (alast[(int64_t)(2 * b) * hl + j] - alast[(int64_t)(2 * b + 1) * hl + j]);
  dwp[j] = acc;
}

// one thread per target occurrence o = 2 b + c (dwide zeroed before): the FIRST occurrence of an id sums every occurrence of it in
// ascending o (+ g coef_b at the positive, - g coef_b at the negative) and writes the id's entry; id 0 is the padding row: no
// gradient.  Every workgroup walks the whole id list through LDS in chunks (item ids fit 32 bits: the catalogue is < 2^31 items).
constexpr int WD_WG_CHUNK = 2048;
__global__ void __launch_bounds__(256) wd_wide_grad_kernel(const int64_t* __restrict__ target, int64_t n_items,
                                                           const float* __restrict__ head, const float* __restrict__ gsd, float gscale,
                                                           int n, float* __restrict__ dwide) {
  __shared__ int ids[WD_WG_CHUNK];
  const int o = blockIdx.x * 256 + threadIdx.x;
  int id = -1;
  if (o < n) {
    const int64_t t = target[o];
    if (t > 0 && t < n_items) id = (int)t;         // padding, or flagged by the forward: skipped
  }
  const float g = gscale * gsd[0];
  bool owner = id > 0;
  float acc = 0.f;
  for (int base = 0; base < n; base += WD_WG_CHUNK) {
    const int m = min(WD_WG_CHUNK, n - base);
    __syncthreads();
    for (int q = threadIdx.x; q < m; q += 256) {
      const int64_t t = target[base + q];
      ids[q] = (t > 0 && t < n_items) ? (int)t : -1;
    }
    __syncthreads();
    if (owner) {
      for (int q = 0; q < m; ++q) {
        if (ids[q] == id) {
          const int gq = base + q;
          if (gq < o) { owner = false; break; }    // an earlier occurrence owns this id
          acc += ((gq & 1) ? -g : g) * head[1 + (gq >> 1)];
        }
      }
    }
  }
  if (owner) dwide[id] = acc;
}

// ---------------------------------------------------------------------------------------------------- evaluation
constexpr int WD_BM = MT_BM;
constexpr int WD_SMEM_FLOATS = 2 * MT_TILE + 3 * 128 + 4;
struct WdRelu {
  __device__ __forceinline__ float operator()(float v) const { return fmaxf(v, 0.f); }
};
constexpr int WD_MAX_H = 128, WD_MAX_L = 64;

struct WdTopkArgs {
  const float* T;                         // [N, h1] = deep W1t^T + b1
  const float* hb;                        // [B, h1] = W1h xh_b
  const float* wide;                      // [N]
  const float* wide_bias; const float* bp;   // [1], [1]
  const int64_t* window;                  // [B, L] left-padded with 0
  const int* hist_ptr;                    // [B + 1] CSR offsets (may be null)
  const int64_t* hist_items;
  const float* w2; const float* b2;       // [h2, h1], [h2] (null with one hidden layer)
  const float* wp;                        // [h_last]
  float* sb;                              // workspace [B]: the per-user scalar
  int* bad;                               // workspace: != 0 once bad input was met
  float* part_val; int* part_idx;         // workspace [B, n_split * 2, KT]
  int32_t* status;
  int B, L, N, h1, h2, tiles_n, n_split;
};

// one wave per user: input checks, s_b = sum_l wide[window[b, l]] (ascending l; padding reads entry 0) + wide_bias + b_p
__global__ void __launch_bounds__(64) wd_prep_kernel(WdTopkArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  bool bad = false;
  for (int l = lane; l < a.L; l += 64) {
    const int64_t id = a.window[(int64_t)b * a.L + l];
    bad |= id < 0 || id >= a.N;
  }
  bad |= hist_ids_bad<64>(a.hist_ptr, a.hist_items, b, a.N, lane);
  if (bad) raise_bad_input(a.bad, a.status);
  if (lane == 0) {
    float s = 0.f;
    for (int l = 0; l < a.L; ++l) {
      const int64_t id = a.window[(int64_t)b * a.L + l];
      if (id >= 0 && id < a.N) s += a.wide[id];
    }
    a.sb[b] = (s + a.wide_bias[0]) + a.bp[0];
  }
}

// KT = length of the top-K lists; TWO = two hidden layers (else one: w_p reads the first layer's activations)
template <int KT, bool TWO>
__global__ void __launch_bounds__(GEMM_THREADS) wd_topk_kernel(WdTopkArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[WD_SMEM_FLOATS];
  if (*a.bad) return;
  float* tile = smem;                          // [128 items][MT_LD] activations
  float* w2s = smem + MT_TILE;                 // W2 [128][MT_LD], zero outside [h2][h1]
  float* wps = w2s + MT_TILE;                  // w_p, zero beyond h_last
  float* b2s = wps + 128;
  float* hbs = b2s + 128;                      // h_b, zero beyond h1
  unsigned* bitmap = reinterpret_cast<unsigned*>(hbs + 128);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = lane >> 5, r = lane & 31;
  const int b = blockIdx.x % a.B, sp = blockIdx.x / a.B;      // user fastest: neighbours share the T tiles
  const TileRange tr = split_tile_range(a.tiles_n, a.n_split, sp);
  const int hl = TWO ? a.h2 : a.h1;
  const int h1 = a.h1;

  mlp_tail_stage<TWO>(w2s, wps, b2s, a.w2, a.b2, a.wp, h1, a.h2, tid);
  if (tid < 128) hbs[tid] = tid < h1 ? a.hb[(int64_t)b * h1 + tid] : 0.f;
  const float sb = a.sb[b];
  const int jstart = tid % hl;                 // mlp_tail_dot: every item thread starts at another column
  const int nb2 = (a.h2 + 31) >> 5, ksteps = (h1 + 7) >> 3;
  const int vper = 2 * ksteps;                 // float4 columns of a tile row that anything reads
  int hb = 0, he = 0;
  if (a.hist_ptr) { hb = a.hist_ptr[b]; he = a.hist_ptr[b + 1]; }
  __syncthreads();

  TopList<KT> top;
  top.init();

  for (int tn = tr.tn0; tn < tr.tn1; ++tn) {
    const int n0 = tn * WD_BM;
    if (tid < 4) bitmap[tid] = 0u;
    // first layer: relu(T[n] + h_b) -> tile (zero beyond h1 and beyond the catalogue)
    for (int e = tid; e < WD_BM * vper; e += GEMM_THREADS) {
      const int rl = e / vper, v = e - rl * vper;
      const int item = n0 + rl, col = 4 * v;
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      if (item < a.N && col < h1) {            // h1 % 4 == 0: a float4 never straddles the row's end
        const float4 tv = *reinterpret_cast<const float4*>(a.T + (int64_t)item * h1 + col);
        const float4 hv = *reinterpret_cast<const float4*>(hbs + col);
        t.x = fmaxf(tv.x + hv.x, 0.f); t.y = fmaxf(tv.y + hv.y, 0.f);
        t.z = fmaxf(tv.z + hv.z, 0.f); t.w = fmaxf(tv.w + hv.w, 0.f);
      }
      *reinterpret_cast<float4*>(tile + rl * MT_LD + col) = t;
    }
    __syncthreads();
    // history mask over the user's FULL history: items of this tile as bits
    hist_bitmap_rows<WD_BM, GEMM_THREADS>(bitmap, a.hist_items, hb, he, n0, tid, [](int) { return 0; });
    if constexpr (TWO) {
      f32x16 acc2[4];
      mlp_tail_layer2(acc2, tile, w2s, ksteps, nb2, wave, r, hh);
      __syncthreads();                         // every wave has read the first layer's activations
      mlp_tail_layer2_store(tile, acc2, b2s, nb2, wave, r, hh, WdRelu{});
    }
    __syncthreads();                           // the last layer's activations and the bitmap are complete
    if (tid < WD_BM) {
      const int item = n0 + tid;
      if (item_alive(bitmap, item, tid, a.N))
        top.insert((sb + a.wide[item]) + mlp_tail_dot(wps, tile + tid * MT_LD, hl, jstart), item);
    }
    __syncthreads();                           // the tile and the bitmap are rewritten by the next item tile
  }
  if (wave >= 2) return;                       // the lists live in the 128 item threads (wave-uniform)
  // the wave's 64 lists -> one list per (user, split, wave)
  const int64_t o = (((int64_t)b * a.n_split + sp) * 2 + wave) * KT;
  wave_collapse_lists(top, lane, a.part_val + o, a.part_idx + o);
}

static int wd_tiles(int N) { return (N + WD_BM - 1) / WD_BM; }
static bool wd_shape_ok(int B, int L, int N, int h1, int h2, int K) {
  return B > 0 && B <= (1 << 20) && L >= 1 && L <= WD_MAX_L && N > 0 && h1 >= 4 && h1 % 4 == 0 && h1 <= WD_MAX_H && h2 >= 0 &&
         h2 <= WD_MAX_H && K >= 1 && K <= 32 && (int64_t)N * h1 * 4 < 0x7FFFFFFFF0ll;
}
static inline bool wd_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline unsigned wd_blocks(int64_t n) {
  int64_t blocks = (n + 255) / 256;
  return (unsigned)(blocks > 65536 ? 65536 : (blocks < 1 ? 1 : blocks));
}

}  // namespace pxr

using namespace pxr;

static int wd_rows_ok(const char* who, int B, int h) {
  PXR_REQUIRE(B > 0 && h > 0 && h <= 4096 && (int64_t)2 * B * h < (1ll << 31), "%s: need B > 0, 0 < h <= 4096 and 2 B h < 2^31", who);
  return PXR_OK;
}

extern "C" int pxr_wd_join_f32(const float* zh, const float* zt, const float* b1, int B, int h1, float* a1, float* der, void* stream) {
  PXR_REQUIRE(zh && zt && b1 && a1 && der, "pxr_wd_join_f32: null pointer");
  if (int rc = wd_rows_ok("pxr_wd_join_f32", B, h1)) return rc;
  const int64_t n = (int64_t)2 * B * h1;
  hipLaunchKernelGGL(wd_join_kernel, dim3(wd_blocks(n)), dim3(256), 0, (hipStream_t)stream, zh, zt, b1, n, h1, a1, der);
  return pxr_check_launch("pxr_wd_join_f32");
}

extern "C" int pxr_wd_join_bwd_f32(const float* dz1, int B, int h1, float* dzh, void* stream) {
  PXR_REQUIRE(dz1 && dzh, "pxr_wd_join_bwd_f32: null pointer");
  if (int rc = wd_rows_ok("pxr_wd_join_bwd_f32", B, h1)) return rc;
  const int64_t n = (int64_t)B * h1;
  hipLaunchKernelGGL(wd_join_bwd_kernel, dim3(wd_blocks(n)), dim3(256), 0, (hipStream_t)stream, dz1, n, h1, dzh);
  return pxr_check_launch("pxr_wd_join_bwd_f32");
}

extern "C" int pxr_wd_head_fwd_f32(const float* alast, const float* wp, const float* wide, int64_t n_items, const int64_t* target,
                                   int B, int hl, float* head, void* stream) {
  PXR_REQUIRE(alast && wp && wide && target && head, "pxr_wd_head_fwd_f32: null pointer");
  PXR_REQUIRE(n_items > 0, "pxr_wd_head_fwd_f32: need n_items > 0");
  if (int rc = wd_rows_ok("pxr_wd_head_fwd_f32", B, hl)) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(wd_head_fwd_kernel, dim3((unsigned)B), dim3(64), 0, st, alast, wp, wide, n_items, target, B, hl, head,
                     pxr_status_word());
  int rc = pxr_check_launch("pxr_wd_head_fwd_f32");
  if (rc) return rc;
  hipLaunchKernelGGL(wd_loss_kernel, dim3(1), dim3(256), 0, st, head, B);
  return pxr_check_launch("pxr_wd_head_fwd_f32 (loss)");
}

extern "C" int pxr_wd_head_bwd_f32(const float* alast, const float* dact, const float* wp, const int64_t* target, int64_t n_items,
                                   const float* head, int B, int hl, float grad_scale, const float* grad_scale_dev, float* dz,
                                   float* dwp, float* dbp, float* dwide, float* dwide_bias, void* stream) {
  PXR_REQUIRE(alast && dact && wp && target && head && grad_scale_dev && dz && dwp && dbp && dwide && dwide_bias,
              "pxr_wd_head_bwd_f32: null pointer");
  PXR_REQUIRE(n_items > 0 && n_items < (1ll << 31), "pxr_wd_head_bwd_f32: need 0 < n_items < 2^31");
  if (int rc = wd_rows_ok("pxr_wd_head_bwd_f32", B, hl)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)2 * B * hl;
  hipLaunchKernelGGL(wd_head_bwd_kernel, dim3(wd_blocks(n)), dim3(256), 0, st, dact, wp, head, grad_scale_dev, grad_scale, n, hl, dz);
  int rc = pxr_check_launch("pxr_wd_head_bwd_f32");
  if (rc) return rc;
  hipLaunchKernelGGL(wd_predict_grad_kernel, dim3((unsigned)((hl + 1 + 63) / 64)), dim3(64), 0, st, alast, head, grad_scale_dev,
                     grad_scale, B, hl, dwp, dbp, dwide_bias);
  rc = pxr_check_launch("pxr_wd_head_bwd_f32 (predict layer)");
  if (rc) return rc;
  if (hipMemsetAsync(dwide, 0, (size_t)n_items * sizeof(float), st) != hipSuccess) return pxr_check_launch("pxr_wd_head_bwd_f32 (memset)");
  hipLaunchKernelGGL(wd_wide_grad_kernel, dim3((unsigned)((2 * B + 255) / 256)), dim3(256), 0, st, target, n_items, head, grad_scale_dev,
                     grad_scale, 2 * B, dwide);
  return pxr_check_launch("pxr_wd_head_bwd_f32 (wide gradient)");
}

// input flag | per-user scalars | partial values | partial ids
extern "C" int64_t pxr_wd_topk_ws_bytes(int B, int L, int N, int h1, int h2, int K) {
  if (!wd_shape_ok(B, L, N, h1, h2, K)) return -1;
  const int64_t cand = (int64_t)topk_pick_split(B, wd_tiles(N)) * 2 * pick_kt(K);
  return topk_ws_bytes(a256((int64_t)B * 4), B, cand);
}

extern "C" int pxr_wd_topk_f32(const float* T, int N, int h1, const float* hb, const int64_t* window, int B, int L, const float* wide,
                               const float* wide_bias, const float* w2, const float* b2, int h2, const float* wp, const float* bp,
                               const int32_t* hist_ptr, const int64_t* hist_items, int K, int64_t* topk_idx, float* topk_val, void* ws,
                               int64_t ws_bytes, void* stream) {
  PXR_REQUIRE(T && hb && window && wide && wide_bias && wp && bp && topk_idx && topk_val && ws, "pxr_wd_topk_f32: null pointer");
  PXR_REQUIRE(wd_shape_ok(B, L, N, h1, h2, K),
              "pxr_wd_topk_f32: outside the fused limits (hidden widths %% 4 == 0 and <= 128, 1 <= L <= 64, 1 <= K <= 32)");
  PXR_REQUIRE(h2 == 0 || (w2 && b2), "pxr_wd_topk_f32: a second hidden layer needs w2 and b2");
  PXR_REQUIRE(wd_aligned(T) && wd_aligned(ws), "pxr_wd_topk_f32: T and the workspace must be 16-byte aligned");
  PXR_REQUIRE(!hist_ptr || hist_items, "pxr_wd_topk_f32: hist_ptr without hist_items");
  if (pxr_wd_topk_ws_bytes(B, L, N, h1, h2, K) > ws_bytes) { pxr_set_error("pxr_wd_topk_f32: workspace too small"); return PXR_ERR_WORKSPACE; }
  const int kt = pick_kt(K);
  WdTopkArgs a{};
  a.T = T; a.hb = hb; a.wide = wide; a.wide_bias = wide_bias; a.bp = bp; a.window = window; a.hist_ptr = hist_ptr;
  a.hist_items = hist_items; a.w2 = w2; a.b2 = b2; a.wp = wp; a.B = B; a.L = L; a.N = N; a.h1 = h1; a.h2 = h2;
  a.tiles_n = wd_tiles(N);
  a.n_split = topk_pick_split(B, a.tiles_n);
  a.status = pxr_status_word();
  const int64_t cand = (int64_t)a.n_split * 2 * kt;
  const TopkWs w = topk_ws_carve(ws, a256((int64_t)B * 4), B, cand);
  a.bad = w.bad; a.part_val = w.part_val; a.part_idx = w.part_idx;
  a.sb = (float*)w.own;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = topk_ws_clear_flag(w, "pxr_wd_topk_f32(memset)", st)) return rc;
  hipLaunchKernelGGL(wd_prep_kernel, dim3((unsigned)B), dim3(64), 0, st, a);
  if (int rc = pxr_check_launch("pxr_wd_topk_f32(prep)")) return rc;
  const dim3 grid((unsigned)(B * a.n_split));
  topk_for_kt(kt, [&](auto k) {
    constexpr int KT = decltype(k)::value;
    if (h2 > 0) hipLaunchKernelGGL((wd_topk_kernel<KT, true>), grid, dim3(GEMM_THREADS), 0, st, a);
    else hipLaunchKernelGGL((wd_topk_kernel<KT, false>), grid, dim3(GEMM_THREADS), 0, st, a);
  });
  return topk_ws_merge(w, B, cand, K, topk_idx, topk_val, "pxr_wd_topk_f32", "pxr_wd_topk_f32(merge)", stream);
}
