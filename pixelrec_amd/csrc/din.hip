// din.hip -- DIN (reference code/REC/model/IDNet/din.py with SequenceAttLayer, layers.py:460-514): target attention over the history.
//
//   per (candidate q, history item k_l):  x = [q | k_l | q - k_l | q * k_l]   ->  MLP with sigmoids  ->  dense (h_last -> 1)  =  s_l
//   s_l = 0 where the window position is padding, then s_l / sqrt(D);      score(q) = sum_l s_l <k_l, q>
//   loss = -mean_b log(sigmoid(score(pos_b) - score(neg_b)) + 1e-8) + 0.01 ||item_emb||_2 / B          (din.py:79-81)
//
// Training side: the attention-input gather, the loss head (forward and backward) and the fold of the MLP's input gradient into
// one gradient row per table occurrence.  The MLP layers themselves are the library GEMMs (EPI_BIAS_ACT_GRAD / ACT_SIGMOID).
// Occurrences: o in [0, B L) = history (b, l); o = B L + 2 b + c = candidate c of sample b (0 positive, 1 negative).
// Pair rows:   r = (c B + b) L + l.   Every sum has one fixed order; no atomics on floats.
//
// Evaluation side (din_topk_kernel): the first Linear factorises,
//   W1 [q | k | q - k | q * k] + b1 = (A q + b1) + Bm k + C (q * k),    A = W1[:, 0:D] + W1[:, 2D:3D],  Bm = W1[:, D:2D] - W1[:, 2D:3D],
//   C = W1[:, 3D:4D]
// so per window row l the pre-activations of a whole item tile are ONE product of the table tile with C scaled by k_l
// (Cs[j, d] = C[j, d] k_l[d], made by din_prep_kernel) plus the per-item term AQ = A q + b1 (made once per evaluation) and the
// per-row term Bm k_l.  A workgroup owns one user and a range of 128-item tiles: per tile and per valid window row it runs the
// fp32-operand MFMA main loop of gemm_f32.cuh (items x h1), applies the sigmoid into an LDS tile, multiplies that tile with W2
// (held in LDS) on the same MFMA, applies the second sigmoid, and 128 threads -- one per item -- finish with dense, 1 / sqrt(D)
// and <k_l, q>, accumulating over l in a register.  Masks (item 0, the ragged edge, the user's full history as a bitmap) and a
// per-thread top-K list follow; the lists are merged by wave shuffles and the shared merge kernel (topk_select.cuh: pxr_topk_merge).
// No [B, L, N, *] value reaches memory.
#include "gemm_f32.cuh"
#include "topk_mlp_tail.cuh"
#include "topk_select.cuh"

namespace pxr {

typedef float df4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float din_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
struct DinSigmoid {
  __device__ __forceinline__ float operator()(float v) const { return din_sigmoid(v); }
};

// ---------------------------------------------------------------------------------------------------- training: attention input
// one workgroup per history occurrence (b, l): emb[o, :] = table[rows[o], :] for the occurrence and (l == 0) the sample's two
// candidates; x[r, :] = [q | k | q - k | q * k] for both candidates
__global__ void __launch_bounds__(64) din_att_input_kernel(const df4* __restrict__ table, const int64_t* __restrict__ rows, int B,
                                                           int L, int dv, df4* __restrict__ emb, df4* __restrict__ x) {
  const int o = blockIdx.x, b = o / L, l = o - b * L;
  const int64_t BL = (int64_t)B * L;
  const df4* k = table + rows[o] * dv;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int64_t oc = BL + 2 * b + c;
    const df4* q = table + rows[oc] * dv;
    df4* xr = x + (((int64_t)c * B + b) * L + l) * 4 * dv;
    for (int v = threadIdx.x; v < dv; v += 64) {
      const df4 qv = q[v], kv = k[v];
      xr[v] = qv;
      xr[dv + v] = kv;
      xr[2 * dv + v] = qv - kv;
      xr[3 * dv + v] = qv * kv;
      if (l == 0) emb[oc * dv + v] = qv;
      if (c == 0) emb[(int64_t)o * dv + v] = kv;
    }
  }
}

struct DinHeadArgs {
  const float* alast;          // [2 B L, hl] activations of the last hidden layer
  const float* dact;           // [2 B L, hl] their derivatives (backward)
  const float* wd;             // [hl] dense.weight
  const float* bd;             // [1]  dense.bias
  const df4* emb;              // [B L + 2 B, dv]
  const int64_t* profile;      // [B, L] (0 = padding)
  float* s;                    // [2 B L] masked and scaled attention weights
  float* kq;                   // [2 B L] <k_l, q_c>
  float* head;                 // [2 + 3 B]: loss | regulariser coefficient | coef [B] | x [B] | ssq [B]
  const float* gsd;            // [1] d loss (device)
  float* dz;                   // [2 B L, hl] gradient of the last pre-activation
  float* dsraw;                // [2 B L] gradient of dense's output
  const df4* dx;               // [2 B L, 4 dv] the MLP's input gradient
  df4* occ;                    // [B L + 2 B, dv] one gradient row per occurrence
  float gscale, sqrt_d;
  int B, L, dv, hl;
};

// one wave per sample: s, <k, q>, the score difference x_b and the sample's share of ||item_emb||^2
__global__ void __launch_bounds__(64) din_head_fwd_kernel(DinHeadArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t BL = (int64_t)a.B * a.L;
  const float bd = a.bd[0];
  float score[2] = {0.f, 0.f};
  float ssq = 0.f;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const df4* q = a.emb + (BL + 2 * b + c) * a.dv;
    for (int v = lane; v < a.dv; v += 64) { const df4 t = q[v]; ssq += t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w; }
    for (int l = 0; l < a.L; ++l) {
      const int64_t r = ((int64_t)c * a.B + b) * a.L + l;
      const df4* k = a.emb + ((int64_t)b * a.L + l) * a.dv;
      float acc = 0.f, dot = 0.f;
      for (int j = lane; j < a.hl; j += 64) acc += a.alast[r * a.hl + j] * a.wd[j];
      for (int v = lane; v < a.dv; v += 64) {
        const df4 kv = k[v], qv = q[v];
        dot += kv.x * qv.x + kv.y * qv.y + kv.z * qv.z + kv.w * qv.w;
        if (c == 0) ssq += kv.x * kv.x + kv.y * kv.y + kv.z * kv.z + kv.w * kv.w;
      }
      acc = wave_sum(acc);
      dot = wave_sum(dot);
      const float sv = a.profile[(int64_t)b * a.L + l] == 0 ? 0.f : (acc + bd) / a.sqrt_d;
      score[c] += sv * dot;
      if (lane == 0) { a.s[r] = sv; a.kq[r] = dot; }
    }
  }
  ssq = wave_sum(ssq);
  if (lane == 0) {
    a.head[2 + a.B + b] = score[0] - score[1];
    a.head[2 + 2 * a.B + b] = ssq;
  }
}

// one workgroup: loss = -mean log(sigmoid(x) + 1e-8) + reg sqrt(sum ssq) / B; coef[b] = d loss / d x_b; head[1] = reg / (B norm)
// (reg: DIN's 0.01, din.py:79; MODIN's 0, modin.py:61 -- head[1] is then +0.0 and the fold adds an exact zero)
__global__ void __launch_bounds__(256) din_loss_kernel(float* __restrict__ head, int B, float reg) {
  __shared__ float red[256];
  float t = 0.f, q = 0.f;
  for (int b = threadIdx.x; b < B; b += 256) {
    const float sg = din_sigmoid(head[2 + B + b]);
    t += logf(sg + 1e-8f);
    q += head[2 + 2 * B + b];
    head[2 + b] = -(1.0f / (float)B) * sg * (1.0f - sg) / (sg + 1e-8f);
  }
  t = block_sum256(t, red);
  q = block_sum256(q, red);
  if (threadIdx.x == 0) {
    const float nrm = sqrtf(q);
    head[0] = -t / (float)B + reg * nrm / (float)B;
    head[1] = nrm > 0.f ? reg / ((float)B * nrm) : 0.f;
  }
}

// dsraw[r] = d loss / d dense(r) (0 at padding); dz[r, j] = dsraw[r] wd[j] act'[r, j]
__global__ void __launch_bounds__(256) din_head_bwd_kernel(DinHeadArgs a) {
  const int64_t n = (int64_t)2 * a.B * a.L * a.hl;
  const float g = a.gscale * a.gsd[0];
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / a.hl;
    const int j = (int)(e - r * a.hl);
    const int64_t cb = r / a.L;
    const int l = (int)(r - cb * a.L);
    const int c = (int)(cb / a.B), b = (int)(cb - (int64_t)c * a.B);
    const bool masked = a.profile[(int64_t)b * a.L + l] == 0;
    const float ds = masked ? 0.f : (c ? -g : g) * a.head[2 + b] * a.kq[r] / a.sqrt_d;
    a.dz[e] = ds * a.wd[j] * a.dact[e];
    if (j == 0) a.dsraw[r] = ds;
  }
}

// block j < hl: dwd[j] = sum_r dsraw[r] alast[r, j]; block hl: dbd = sum_r dsraw[r]   (fixed order)
__global__ void __launch_bounds__(256) din_dense_grad_kernel(const float* __restrict__ dsraw, const float* __restrict__ alast,
                                                             int64_t R, int hl, float* __restrict__ dwd, float* __restrict__ dbd) {
  __shared__ float red[256];
  const int j = blockIdx.x;
  float t = 0.f;
  for (int64_t r = threadIdx.x; r < R; r += 256) t += j < hl ? dsraw[r] * alast[r * hl + j] : dsraw[r];
  t = block_sum256(t, red);
  if (threadIdx.x == 0) {
    if (j < hl) dwd[j] = t;
    else dbd[0] = t;
  }
}

// one workgroup per occurrence: the gradient row of the table occurrence (direct path through the score, the MLP's input gradient
// folded through [q | k | q - k | q * k], the regulariser)
__global__ void __launch_bounds__(64) din_fold_bwd_kernel(DinHeadArgs a) {
  const int64_t o = blockIdx.x, BL = (int64_t)a.B * a.L;
  const int dv = a.dv;
  const float g = a.gscale * a.gsd[0];
  const float reg = g * a.head[1];
  df4* out = a.occ + o * dv;
  if (o < BL) {
    const int b = (int)(o / a.L), l = (int)(o - (int64_t)b * a.L);
    const bool masked = a.profile[o] == 0;
    const df4* k = a.emb + o * dv;
    for (int v = threadIdx.x; v < dv; v += 64) {
      df4 acc = reg * k[v];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int64_t r = ((int64_t)c * a.B + b) * a.L + l;
        const df4 q = a.emb[(BL + 2 * b + c) * dv + v];
        const df4* dxr = a.dx + r * 4 * dv;
        const float gc = (c ? -g : g) * a.head[2 + b] * a.s[r];
        acc += gc * q + dxr[dv + v] - dxr[2 * dv + v] + dxr[3 * dv + v] * q;
      }
      out[v] = masked ? df4{0.f, 0.f, 0.f, 0.f} : acc;
    }
  } else {
    const int64_t i = o - BL;
    const int b = (int)(i >> 1), c = (int)(i & 1);
    const float gc = (c ? -g : g) * a.head[2 + b];
    const df4* q = a.emb + o * dv;
    for (int v = threadIdx.x; v < dv; v += 64) {
      df4 acc = reg * q[v];
      for (int l = 0; l < a.L; ++l) {
        const int64_t r = ((int64_t)c * a.B + b) * a.L + l;
        const df4 k = a.emb[((int64_t)b * a.L + l) * dv + v];
        const df4* dxr = a.dx + r * 4 * dv;
        acc += (gc * a.s[r]) * k + dxr[v] + dxr[2 * dv + v] + dxr[3 * dv + v] * k;
      }
      out[v] = acc;
    }
  }
}

// ---------------------------------------------------------------------------------------------------- evaluation
// A | Bm | C [h1, D] each from W1 [h1, 4 D]
__global__ void __launch_bounds__(256) din_fold_w1_kernel(const float* __restrict__ w1, int h1, int D, float* __restrict__ A,
                                                          float* __restrict__ Bm, float* __restrict__ C) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= h1 * D) return;
  const int j = e / D, d = e - j * D;
  const float* w = w1 + (int64_t)j * 4 * D;
  A[e] = w[d] + w[2 * D + d];
  Bm[e] = w[D + d] - w[2 * D + d];
  C[e] = w[3 * D + d];
}

constexpr int DN_BM = MT_BM, DN_BN = 128;
using DnCfg = GemmCfg<DN_BM, DN_BN, true, true>;
constexpr int DN_SMEM_FLOATS = 2 * MT_TILE + 3 * 128 + 4;
constexpr int DN_MAX_D = 128, DN_MAX_H = 128, DN_MAX_L = 64;

struct DinTopkArgs {
  const float* table;                     // [N, D]
  const int64_t* window;                  // [B, L] left-padded with 0
  const int* hist_ptr;                    // [B + 1] CSR offsets (may be null)
  const int64_t* hist_items;
  const float* aq;                        // [N, h1] = A q_n + b1
  const float* bm;                        // [h1, D]
  const float* cm;                        // [h1, D]
  const float* w2; const float* b2;       // [h2, h1], [h2] (null with one hidden layer)
  const float* wd; const float* bd;       // [h_last], [1]
  float* cs;                              // workspace [B L, h1, D]: C scaled by the window row
  float* bk;                              // workspace [B L, 128]: Bm k_l (zero beyond h1)
  int* bad;                               // workspace: != 0 once bad input was met
  float* part_val; int* part_idx;         // workspace [B, n_split * 2, KT]
  int32_t* status;
  float sqrt_d;
  int B, L, N, D, h1, h2, tiles_n, n_split;
};

// one workgroup per window position: input checks, Cs = C * k_l, Bk = Bm k_l
__global__ void __launch_bounds__(256) din_prep_kernel(DinTopkArgs a) {
  const int bl = blockIdx.x, b = bl / a.L, l = bl - b * a.L, tid = threadIdx.x;
  const int64_t id = a.window[bl];
  bool bad = id < 0 || id >= a.N;
  if (l == 0) bad |= hist_ids_bad<256>(a.hist_ptr, a.hist_items, b, a.N, tid);
  if (bad) raise_bad_input(a.bad, a.status);
  if (id <= 0 || id >= a.N) return;            // padding (or flagged): this row takes no part
  const float* k = a.table + id * a.D;
  float* cs = a.cs + (int64_t)bl * a.h1 * a.D;
  const int n = a.h1 * a.D;
  for (int e = tid; e < n; e += 256) cs[e] = a.cm[e] * k[e % a.D];
  if (tid < 128) {
    float acc = 0.f;
    if (tid < a.h1)
      for (int d = 0; d < a.D; ++d) acc += a.bm[tid * a.D + d] * k[d];
    a.bk[(int64_t)bl * 128 + tid] = acc;
  }
}

// KT = length of the top-K lists; TWO = two hidden layers (else one: dense reads the first layer's activations)
template <int KT, bool TWO>
__global__ void __launch_bounds__(GEMM_THREADS) din_topk_kernel(DinTopkArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[DN_SMEM_FLOATS];
  if (*a.bad) return;
  float* tile = smem;                          // staging buffers of the main loop, then the [128 items][MT_LD] activations
  float* w2s = smem + MT_TILE;                 // W2 [128][MT_LD], zero outside [h2][h1]
  float* wds = w2s + MT_TILE;                  // dense.weight, zero beyond h_last
  float* b2s = wds + 128;
  float* ks = b2s + 128;                       // the window row k_l
  unsigned* bitmap = reinterpret_cast<unsigned*>(ks + 128);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, hh = lane >> 5, r = lane & 31;
  const int b = blockIdx.x % a.B, sp = blockIdx.x / a.B;      // user fastest: neighbours share the item tiles
  const TileRange tr = split_tile_range(a.tiles_n, a.n_split, sp);
  const int hl = TWO ? a.h2 : a.h1;
  const int D = a.D, h1 = a.h1;

  mlp_tail_stage<TWO>(w2s, wds, b2s, a.w2, a.b2, a.wd, h1, a.h2, tid);
  const float bd = a.bd[0];
  const int jstart = tid % hl;                 // mlp_tail_dot: every item thread starts at another column
  const int nb2 = (a.h2 + 31) >> 5, ksteps = (h1 + 7) >> 3;
  int hb = 0, he = 0;
  if (a.hist_ptr) { hb = a.hist_ptr[b]; he = a.hist_ptr[b + 1]; }
  const int64_t* win = a.window + (int64_t)b * a.L;

  TopList<KT> top;
  top.init();

  for (int tn = tr.tn0; tn < tr.tn1; ++tn) {
    const int n0 = tn * DN_BM;
    if (tid < 4) bitmap[tid] = 0u;
    // the per-item term A q + b1 of this tile, in the accumulator layout: read once per tile, used by every window row
    float aqr[DnCfg::TM][DnCfg::TN][16];
#pragma unroll
    for (int j = 0; j < DnCfg::TN; ++j) {
      const int col = wn * DnCfg::WN + j * 32 + r;
#pragma unroll
      for (int i = 0; i < DnCfg::TM; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = n0 + wm * DnCfg::WM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
          aqr[i][j][e] = (row < a.N && col < h1) ? a.aq[(int64_t)row * h1 + col] : 0.f;
        }
    }
    __syncthreads();
    // history mask over the user's FULL history: items of this tile as bits
    hist_bitmap_rows<DN_BM, GEMM_THREADS>(bitmap, a.hist_items, hb, he, n0, tid, [](int) { return 0; });
    float score = 0.f;
    for (int l = 0; l < a.L; ++l) {
      const int64_t w = win[l];
      if (w == 0) continue;                    // padding: s = 0 exactly (workgroup-uniform)
      const int64_t bl = (int64_t)b * a.L + l;
      if (tid < D) ks[tid] = a.table[w * D + tid];
      typename DnCfg::Acc accs;
      gemm_mainloop<DN_BM, DN_BN, true, true, false, 1, 2, 2, 0, false, false>(accs, a.table, (int64_t)D, a.cs + bl * h1 * D, (int64_t)D,
                                                                               a.N, h1, 0, D, n0, 0, smem);
      // (the main loop ends with a barrier: the staging buffers are free)  first sigmoid -> tile
#pragma unroll
      for (int j = 0; j < DnCfg::TN; ++j) {
        const int col = wn * DnCfg::WN + j * 32 + r;
        const float bkv = a.bk[bl * 128 + col];
#pragma unroll
        for (int i = 0; i < DnCfg::TM; ++i)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int rl = wm * DnCfg::WM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
            tile[rl * MT_LD + col] = din_sigmoid(accs.v[i][j][e] + aqr[i][j][e] + bkv);
          }
      }
      __syncthreads();
      if constexpr (TWO) {
        f32x16 acc2[4];
        mlp_tail_layer2(acc2, tile, w2s, ksteps, nb2, wave, r, hh);
        __syncthreads();                       // every wave has read the first layer's activations
        mlp_tail_layer2_store(tile, acc2, b2s, nb2, wave, r, hh, DinSigmoid{});
        __syncthreads();
      }
      if (tid < DN_BM) {
        const float s = (mlp_tail_dot(wds, tile + tid * MT_LD, hl, jstart) + bd) / a.sqrt_d;
        const int item = n0 + tid;
        if (item < a.N) {
          const float4* q = reinterpret_cast<const float4*>(a.table + (int64_t)item * D);
          float dot = 0.f;
          for (int v = 0; v < D / 4; ++v) {
            const float4 qv = q[v];
            dot += ks[4 * v] * qv.x + ks[4 * v + 1] * qv.y + ks[4 * v + 2] * qv.z + ks[4 * v + 3] * qv.w;
          }
          score += s * dot;
        }
      }
      __syncthreads();                         // the tile and k_l are rewritten by the next window row
    }
    __syncthreads();                           // (an all-padding window: the bitmap still has to be complete)
    if (tid < DN_BM) {
      if (item_alive(bitmap, n0 + tid, tid, a.N)) top.insert(score, n0 + tid);
    }
    __syncthreads();
  }
  if (wave >= 2) return;                       // the lists live in the 128 item threads (wave-uniform)
  // the wave's 64 lists -> one list per (user, split, wave)
  const int64_t o = (((int64_t)b * a.n_split + sp) * 2 + wave) * KT;
  wave_collapse_lists(top, lane, a.part_val + o, a.part_idx + o);
}

static int dn_tiles(int N) { return (N + DN_BM - 1) / DN_BM; }
static int64_t dn_bk_bytes(int B, int L) { return a256((int64_t)B * L * 128 * 4); }
static int64_t dn_own_bytes(int B, int L, int h1, int D) { return dn_bk_bytes(B, L) + a256((int64_t)B * L * h1 * D * 4); }
static bool dn_shape_ok(int B, int L, int N, int D, int h1, int h2, int K) {
  return B > 0 && B <= (1 << 20) && L >= 1 && L <= DN_MAX_L && N > 0 && D >= 4 && D % 4 == 0 && D <= DN_MAX_D && h1 >= 1 &&
         h1 <= DN_MAX_H && h2 >= 0 && h2 <= DN_MAX_H && K >= 1 && K <= 32 && (int64_t)N * D * 4 < 0x7FFFFFF0ll;
}
static inline bool dn_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace pxr

using namespace pxr;

extern "C" int pxr_din_att_input_f32(const float* table, const int64_t* rows, int B, int L, int D, float* emb, float* x,
                                     void* stream) {
  PXR_REQUIRE(table && rows && emb && x, "pxr_din_att_input_f32: null pointer");
  PXR_REQUIRE(B > 0 && L > 0 && (int64_t)2 * B * L < (1ll << 31), "pxr_din_att_input_f32: need B > 0, L > 0 and 2 B L < 2^31");
  PXR_REQUIRE(D > 0 && D % 4 == 0 && D <= 4096, "pxr_din_att_input_f32: need D %% 4 == 0 and 0 < D <= 4096 (D=%d)", D);
  PXR_REQUIRE(dn_aligned(table) && dn_aligned(emb) && dn_aligned(x), "pxr_din_att_input_f32: operands must be 16-byte aligned");
  hipLaunchKernelGGL(din_att_input_kernel, dim3((unsigned)(B * L)), dim3(64), 0, (hipStream_t)stream, (const df4*)table, rows, B, L,
                     D / 4, (df4*)emb, (df4*)x);
  return pxr_check_launch("pxr_din_att_input_f32");
}

static int din_head_shape_ok(const char* who, int B, int L, int D, int hl) {
  PXR_REQUIRE(B > 0 && L > 0 && (int64_t)2 * B * L * (hl > 0 ? hl : 1) < (1ll << 31), "%s: need B > 0, L > 0 and 2 B L h < 2^31", who);
  PXR_REQUIRE(D > 0 && D % 4 == 0 && D <= 4096, "%s: need D %% 4 == 0 and 0 < D <= 4096 (D=%d)", who, D);
  PXR_REQUIRE(hl > 0 && hl <= 4096, "%s: need 0 < h_last <= 4096 (h_last=%d)", who, hl);
  return PXR_OK;
}

// The head with the regulariser's weight as an argument: loss = -mean log(sigmoid(x) + 1e-8) + reg ||emb||_2 / B, head[1] =
// reg / (B ||emb||_2) (0 when reg == 0 or the norm is 0).  The head layout does not depend on reg.
extern "C" int pxr_din_head_fwd_reg_f32(const float* alast, const float* wd, const float* bd, const float* emb, const int64_t* profile,
                                        int B, int L, int D, int hl, float* s, float* kq, float* head, float reg,
                                        void* stream) {
  PXR_REQUIRE(alast && wd && bd && emb && profile && s && kq && head, "pxr_din_head_fwd_reg_f32: null pointer");
  if (int rc = din_head_shape_ok("pxr_din_head_fwd_reg_f32", B, L, D, hl)) return rc;
  PXR_REQUIRE(reg >= 0.f && reg < INFINITY, "pxr_din_head_fwd_reg_f32: reg must be finite and >= 0");
  PXR_REQUIRE(dn_aligned(emb), "pxr_din_head_fwd_reg_f32: emb must be 16-byte aligned");
  DinHeadArgs a{};
  a.alast = alast; a.wd = wd; a.bd = bd; a.emb = (const df4*)emb; a.profile = profile; a.s = s; a.kq = kq; a.head = head;
  a.B = B; a.L = L; a.dv = D / 4; a.hl = hl; a.sqrt_d = sqrtf((float)D);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(din_head_fwd_kernel, dim3((unsigned)B), dim3(64), 0, st, a);
  int rc = pxr_check_launch("pxr_din_head_fwd_reg_f32");
  if (rc) return rc;
  hipLaunchKernelGGL(din_loss_kernel, dim3(1), dim3(256), 0, st, head, B, reg);
  return pxr_check_launch("pxr_din_head_fwd_reg_f32 (loss)");
}

// DIN's head: the regulariser of din.py:79
extern "C" int pxr_din_head_fwd_f32(const float* alast, const float* wd, const float* bd, const float* emb, const int64_t* profile,
                                    int B, int L, int D, int hl, float* s, float* kq, float* head, void* stream) {
  return pxr_din_head_fwd_reg_f32(alast, wd, bd, emb, profile, B, L, D, hl, s, kq, head, 0.01f, stream);
}

extern "C" int pxr_din_head_bwd_f32(const float* alast, const float* dact, const float* wd, const int64_t* profile, const float* kq,
                                    const float* head, int B, int L, int D, int hl, float grad_scale, const float* grad_scale_dev,
                                    float* dz, float* dsraw, float* dwd, float* dbd, void* stream) {
  PXR_REQUIRE(alast && dact && wd && profile && kq && head && grad_scale_dev && dz && dsraw && dwd && dbd,
              "pxr_din_head_bwd_f32: null pointer");
  if (int rc = din_head_shape_ok("pxr_din_head_bwd_f32", B, L, D, hl)) return rc;
  DinHeadArgs a{};
  a.alast = alast; a.dact = dact; a.wd = wd; a.profile = profile; a.kq = (float*)kq; a.head = (float*)head; a.gsd = grad_scale_dev;
  a.dz = dz; a.dsraw = dsraw; a.gscale = grad_scale; a.B = B; a.L = L; a.dv = D / 4; a.hl = hl; a.sqrt_d = sqrtf((float)D);
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)2 * B * L * hl;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(din_head_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
  int rc = pxr_check_launch("pxr_din_head_bwd_f32");
  if (rc) return rc;
  hipLaunchKernelGGL(din_dense_grad_kernel, dim3((unsigned)(hl + 1)), dim3(256), 0, st, (const float*)dsraw, alast, (int64_t)2 * B * L,
                     hl, dwd, dbd);
  return pxr_check_launch("pxr_din_head_bwd_f32 (dense gradient)");
}

extern "C" int pxr_din_fold_bwd_f32(const float* dx, const float* emb, const int64_t* profile, const float* s, const float* head,
                                    int B, int L, int D, float grad_scale, const float* grad_scale_dev, float* occ, void* stream) {
  PXR_REQUIRE(dx && emb && profile && s && head && grad_scale_dev && occ, "pxr_din_fold_bwd_f32: null pointer");
  if (int rc = din_head_shape_ok("pxr_din_fold_bwd_f32", B, L, D, 1)) return rc;
  PXR_REQUIRE(dn_aligned(dx) && dn_aligned(emb) && dn_aligned(occ), "pxr_din_fold_bwd_f32: operands must be 16-byte aligned");
  DinHeadArgs a{};
  a.dx = (const df4*)dx; a.emb = (const df4*)emb; a.profile = profile; a.s = (float*)s; a.head = (float*)head; a.gsd = grad_scale_dev;
  a.occ = (df4*)occ; a.gscale = grad_scale; a.B = B; a.L = L; a.dv = D / 4; a.hl = 1;
  hipLaunchKernelGGL(din_fold_bwd_kernel, dim3((unsigned)(B * (L + 2))), dim3(64), 0, (hipStream_t)stream, a);
  return pxr_check_launch("pxr_din_fold_bwd_f32");
}

extern "C" int pxr_din_fold_w1_f32(const float* w1, int h1, int D, float* A, float* Bm, float* C, void* stream) {
  PXR_REQUIRE(w1 && A && Bm && C, "pxr_din_fold_w1_f32: null pointer");
  PXR_REQUIRE(h1 > 0 && D > 0 && (int64_t)h1 * D < (1ll << 28), "pxr_din_fold_w1_f32: bad shape");
  hipLaunchKernelGGL(din_fold_w1_kernel, dim3((unsigned)((h1 * D + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w1, h1, D, A, Bm, C);
  return pxr_check_launch("pxr_din_fold_w1_f32");
}

// input flag | Bm k | C * k | partial values | partial ids
extern "C" int64_t pxr_din_topk_ws_bytes(int B, int L, int N, int D, int h1, int h2, int K) {
  if (!dn_shape_ok(B, L, N, D, h1, h2, K)) return -1;
  const int64_t cand = (int64_t)topk_pick_split(B, dn_tiles(N)) * 2 * pick_kt(K);
  return topk_ws_bytes(dn_own_bytes(B, L, h1, D), B, cand);
}

extern "C" int pxr_din_topk_f32(const float* table, int N, int D, const int64_t* window, int B, int L, const float* aq,
                                const float* bm, const float* cm, int h1, const float* w2, const float* b2, int h2, const float* wd,
                                const float* bd, const int32_t* hist_ptr, const int64_t* hist_items, int K, int64_t* topk_idx,
                                float* topk_val, void* ws, int64_t ws_bytes, void* stream) {
  PXR_REQUIRE(table && window && aq && bm && cm && wd && bd && topk_idx && topk_val && ws, "pxr_din_topk_f32: null pointer");
  PXR_REQUIRE(dn_shape_ok(B, L, N, D, h1, h2, K),
              "pxr_din_topk_f32: outside the fused limits (D %% 4 == 0, D <= 128, hidden widths <= 128, 1 <= L <= 64, 1 <= K <= 32)");
  PXR_REQUIRE(h2 == 0 || (w2 && b2), "pxr_din_topk_f32: a second hidden layer needs w2 and b2");
  PXR_REQUIRE(dn_aligned(table) && dn_aligned(ws), "pxr_din_topk_f32: table and workspace must be 16-byte aligned");
  PXR_REQUIRE(!hist_ptr || hist_items, "pxr_din_topk_f32: hist_ptr without hist_items");
  if (pxr_din_topk_ws_bytes(B, L, N, D, h1, h2, K) > ws_bytes) { pxr_set_error("pxr_din_topk_f32: workspace too small"); return PXR_ERR_WORKSPACE; }
  const int kt = pick_kt(K);
  DinTopkArgs a{};
  a.table = table; a.window = window; a.hist_ptr = hist_ptr; a.hist_items = hist_items; a.aq = aq; a.bm = bm; a.cm = cm;
  a.w2 = w2; a.b2 = b2; a.wd = wd; a.bd = bd; a.B = B; a.L = L; a.N = N; a.D = D; a.h1 = h1; a.h2 = h2;
  a.tiles_n = dn_tiles(N);
  a.n_split = topk_pick_split(B, a.tiles_n);
  a.status = pxr_status_word();
  a.sqrt_d = sqrtf((float)D);
  const int64_t cand = (int64_t)a.n_split * 2 * kt;
  const TopkWs w = topk_ws_carve(ws, dn_own_bytes(B, L, h1, D), B, cand);
  a.bad = w.bad; a.part_val = w.part_val; a.part_idx = w.part_idx;
  a.bk = (float*)w.own;
  a.cs = (float*)(w.own + dn_bk_bytes(B, L));
  hipStream_t st = (hipStream_t)stream;
  if (int rc = topk_ws_clear_flag(w, "pxr_din_topk_f32(memset)", st)) return rc;
  hipLaunchKernelGGL(din_prep_kernel, dim3((unsigned)(B * L)), dim3(256), 0, st, a);
  if (int rc = pxr_check_launch("pxr_din_topk_f32(prep)")) return rc;
  const dim3 grid((unsigned)(B * a.n_split));
  topk_for_kt(kt, [&](auto k) {
    constexpr int KT = decltype(k)::value;
    if (h2 > 0) hipLaunchKernelGGL((din_topk_kernel<KT, true>), grid, dim3(GEMM_THREADS), 0, st, a);
    else hipLaunchKernelGGL((din_topk_kernel<KT, false>), grid, dim3(GEMM_THREADS), 0, st, a);
  });
  return topk_ws_merge(w, B, cand, K, topk_idx, topk_val, "pxr_din_topk_f32", "pxr_din_topk_f32(merge)", stream);
}
