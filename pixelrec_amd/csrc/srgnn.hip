// srgnn.hip -- SRGNN (reference code/REC/model/IDNet/srgnn.py, the session graph of collate_fn.graph_train_collate): the graph
// build on the device at a fixed size, the propagation of the gated GNN cell, the attention readout and the pair loss head.
// The matrix products around them (edge Linears, W_ih / W_hh, linear_one|two, linear_transform) are pxr_gemm_f32 / pxr_linear_*
// calls and the gates are gru.hip's; nothing here uses float atomics, so every output is bit-identical from run to run.
//
// Session graph of a sequence x[0..L-1] (right-padded with 0), padded to L nodes instead of the batch's largest node count:
//   nodes  = the distinct ids of x ascending (0 included when x is padded), then 0 up to L slots; alias[t] = index of x[t]
//   edges  = x[i] -> x[i+1] for i + 1 < s, s = the first j >= 1 with x[j] == 0 (the collate's `break`); a repeat counts once
//   A      = [A_in | A_out] [L, 2L]: A_in[v][u] = edge(u, v) / indeg(v), A_out[u][v] = edge(u, v) / outdeg(u) (degree 0 -> 1)
// A padding node has no edges: zero rows and columns, so no output it does not own changes.
#include "pair_head.cuh"

namespace pxr {


constexpr int SRGNN_MAX_L = 64;

// ---------------------------------------------------------------- graph build: one wave per session
struct GraphArgs {
  const int64_t* seq;      // [B, L]
  const int64_t* target;   // [B, 2] or NULL
  int64_t B, n_items;
  int L;
  int64_t* nodes;          // [B, L]
  int32_t* alias;          // [B, L]
  float* A;                // [B, L, 2L]
  int64_t* occ;            // [B, 3L] or NULL: nodes | target, 0.. | negative, 0..  (the occurrence sort's id rows)
  int64_t* mask;           // [B, L] or NULL: x[t] != 0
  int32_t* status;
};

__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int src) {
  const unsigned lo = __shfl((unsigned)(v & 0xffffffffull), src), hi = __shfl((unsigned)(v >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ void __launch_bounds__(256) srgnn_graph_kernel(GraphArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;                                  // (uniform per wave)
  const int L = a.L;
  const bool live = lane < L;
  int x = 0;
  if (live) x = (int)checked_id(a.seq[b * L + lane], a.n_items, a.status, true);
  // first occurrences, then rank = number of distinct ids below x (np.unique order)
  bool first = live;
  for (int j = 0; j < L; ++j) {
    const int xj = __shfl(x, j);
    if (j < lane && xj == x) first = false;
  }
  const unsigned long long fm = __ballot(first);
  int rank = 0;
  for (int j = 0; j < L; ++j) {
    const int xj = __shfl(x, j);
    if (((fm >> j) & 1ull) && xj < x) ++rank;
  }
  const int n_unique = __popcll(fm);
  const unsigned long long zm = __ballot(live && lane >= 1 && x == 0);
  const int s = zm ? (int)__builtin_ctzll(zm) : L;       // edges i -> i+1 for i + 1 < s
  unsigned long long inm = 0, outm = 0;                  // lane r = node r: its predecessors / successors
  for (int i = 0; i + 1 < s; ++i) {
    const int ai = __shfl(rank, i), aj = __shfl(rank, i + 1);
    if (ai == lane) outm |= 1ull << aj;
    if (aj == lane) inm |= 1ull << ai;
  }
  const int din = __popcll(inm), dout = __popcll(outm);
  const float rin = 1.0f / (float)(din ? din : 1), rout = 1.0f / (float)(dout ? dout : 1);
  if (live) {
    if (first) a.nodes[b * L + rank] = x;
    if (lane >= n_unique) a.nodes[b * L + lane] = 0;
    a.alias[b * L + lane] = rank;
    if (a.mask) a.mask[b * L + lane] = x != 0 ? 1 : 0;
    if (a.occ) {
      int64_t* o = a.occ + b * 3 * L;
      if (first) o[rank] = x;
      if (lane >= n_unique) o[lane] = 0;
      o[L + lane] = lane == 0 ? a.target[2 * b] : 0;
      o[2 * L + lane] = lane == 0 ? a.target[2 * b + 1] : 0;
    }
  }
  // rows of A, one per pass: lane c writes columns c and L + c (coalesced)
  float* Ab = a.A + b * (int64_t)L * 2 * L;
  for (int r = 0; r < L; ++r) {
    const unsigned long long ir = shfl_u64(inm, r), orr = shfl_u64(outm, r);
    const float fi = __shfl(rin, r), fo = __shfl(rout, r);
    if (live) {
      Ab[(int64_t)r * 2 * L + lane] = ((ir >> lane) & 1ull) ? fi : 0.f;
      Ab[(int64_t)r * 2 * L + L + lane] = ((orr >> lane) & 1ull) ? fo : 0.f;
    }
  }
}

// ---------------------------------------------------------------- propagation: one workgroup per session, A in LDS
// forward  (transpose 0): y[v, hD + c] = sum_u A[v][hL + u] x[u, hD + c] (+ bias[hD + c])   -- [A_in E_in + b_iah | A_out E_out + b_oah]
// backward (transpose 1): y[u, hD + c] = sum_v A[v][hL + u] x[v, hD + c]                     -- the gradient of the above w.r.t. E
// Sums run over the L nodes in ascending order.  8 output rows per pass keep 8 float4 accumulators in registers.
__global__ void __launch_bounds__(256) srgnn_prop_kernel(const float* __restrict__ A, int L, int D, const float* __restrict__ x,
                                                         float* __restrict__ y, const float* __restrict__ bias, int transpose) {
  extern __shared__ float sA[];                          // [L][2L]
  const int64_t b = blockIdx.x;
  const float* Ab = A + b * (int64_t)L * 2 * L;
  for (int i = threadIdx.x; i < 2 * L * L; i += blockDim.x) sA[i] = Ab[i];
  __syncthreads();
  const int dv = D / 4, n_chunks = 2 * dv;
  const f32x4* xb = reinterpret_cast<const f32x4*>(x + b * (int64_t)L * 2 * D);
  f32x4* yb = reinterpret_cast<f32x4*>(y + b * (int64_t)L * 2 * D);
  for (int q = threadIdx.x; q < n_chunks; q += blockDim.x) {
    const int h = q >= dv ? 1 : 0;
    const f32x4 bv = bias ? reinterpret_cast<const f32x4*>(bias)[q] : f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i0 = 0; i0 < L; i0 += 8) {
      f32x4 acc[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < L; ++j) {
        const f32x4 xv = xb[(int64_t)j * n_chunks + q];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int i = i0 + k;
          if (i < L) {
            const float m = transpose ? sA[j * 2 * L + h * L + i] : sA[i * 2 * L + h * L + j];
            acc[k] += m * xv;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int i = i0 + k;
        if (i < L) yb[(int64_t)i * n_chunks + q] = acc[k] + bv;
      }
    }
  }
}

// ---------------------------------------------------------------- readout (srgnn.py seq_modeling after the GNN)
// Node space: Hn [B*L, D] final node states; P [B*L, 2D] = [Hn W1^T + b1 | Hn W2^T + b2] (one GEMM).  Position t reads node
// alias[t]; ht = position last = sum(mask) - 1, wrapped like torch indexing when the history is empty (-1 -> L-1).
//   s_t = sigmoid(P1[alias[last]] + P2[alias[t]]),  alpha_t = <w3, s_t>,  a = sum_t (alpha_t sh_t) mask_t,  cat = [a | ht]
__device__ __forceinline__ int srgnn_last(const int64_t* mask, int L) {
  int64_t n = 0;
  for (int t = 0; t < L; ++t) n += mask[t];
  int64_t last = n - 1;
  if (last < 0) last += L;                               // torch: index -1 is the last slot
  return (int)(last < 0 ? 0 : (last >= L ? L - 1 : last));
}

__device__ __forceinline__ f32x4 sigmoid4(const f32x4& v) {
  return f32x4{1.f / (1.f + expf(-v.x)), 1.f / (1.f + expf(-v.y)), 1.f / (1.f + expf(-v.z)), 1.f / (1.f + expf(-v.w))};
}


struct ReadoutArgs {
  const float* Hn;         // [B*L, D]
  const float* P;          // [B*L, 2D]
  const int32_t* alias;    // [B, L]
  const int64_t* mask;     // [B, L]
  const float* w3;         // [D]
  int L, D;
  float* cat;              // [B, 2D]
  float* sig;              // [B, L, D] or NULL (saved s_t)
  float* alpha;            // [B, L] or NULL
  // backward
  const float* dcat;       // [B, 2D]
  float* dP;               // [B*L, 2D]
  float* dH;               // [B*L, D]
  float* dw3p;             // [B, D]: the session's part of d w3
};

__global__ void __launch_bounds__(256) srgnn_readout_fwd_kernel(ReadoutArgs a) {
  __shared__ int s_alias[SRGNN_MAX_L];
  __shared__ float s_alpha[SRGNN_MAX_L];
  __shared__ int s_last;
  const int64_t b = blockIdx.x;
  const int L = a.L, dv = a.D / 4, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < L) {
    int al = a.alias[b * L + threadIdx.x];
    s_alias[threadIdx.x] = al < 0 ? 0 : (al >= L ? L - 1 : al);
  }
  if (threadIdx.x == 0) s_last = srgnn_last(a.mask + b * L, L);
  __syncthreads();
  const int64_t nb = b * L;
  const int al = s_alias[s_last];
  const f32x4* P = reinterpret_cast<const f32x4*>(a.P);
  const f32x4* H = reinterpret_cast<const f32x4*>(a.Hn);
  const f32x4* w3 = reinterpret_cast<const f32x4*>(a.w3);
  for (int t = wave; t < L; t += 4) {
    const int64_t rq1 = (nb + al) * 2 * dv, rq2 = (nb + s_alias[t]) * 2 * dv + dv;
    float d = 0.f;
    for (int c = lane; c < dv; c += 64) {
      const f32x4 sv = sigmoid4(P[rq1 + c] + P[rq2 + c]);
      if (a.sig) reinterpret_cast<f32x4*>(a.sig)[(b * L + t) * dv + c] = sv;
      d += dot4(w3[c], sv);
    }
    d = wave_sum(d);
    if (lane == 0) {
      s_alpha[t] = d;
      if (a.alpha) a.alpha[b * L + t] = d;
    }
  }
  __syncthreads();
  f32x4* cat = reinterpret_cast<f32x4*>(a.cat) + b * 2 * dv;
  for (int c = threadIdx.x; c < dv; c += blockDim.x) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < L; ++t) acc += (s_alpha[t] * H[(nb + s_alias[t]) * dv + c]) * (float)a.mask[b * L + t];
    cat[c] = acc;
    cat[dv + c] = H[(nb + al) * dv + c];
  }
}

// Backward: dcat = [da | dht] ->
//   dalpha_t = mask_t <da, sh_t>,  dpre_t = dalpha_t w3 s_t (1 - s_t)
//   dP2[j] = sum_{t: alias t = j} dpre_t,  dP1[alias[last]] = sum_t dpre_t (0 elsewhere)
//   dH[j]  = sum_{t: alias t = j} (alpha_t da) mask_t  (+ dht at j = alias[last])
//   dw3p[b] = sum_t dalpha_t s_t
// Every node's sums run over its positions in ascending order (a counting sort of alias in LDS): no atomics.
__global__ void __launch_bounds__(256) srgnn_readout_bwd_kernel(ReadoutArgs a) {
  __shared__ int s_alias[SRGNN_MAX_L];
  __shared__ float s_alpha[SRGNN_MAX_L], s_dalpha[SRGNN_MAX_L], s_mask[SRGNN_MAX_L];
  __shared__ int s_perm[SRGNN_MAX_L], s_start[SRGNN_MAX_L + 1];
  __shared__ int s_last;
  const int64_t b = blockIdx.x;
  const int L = a.L, dv = a.D / 4, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < L) {
    int al = a.alias[b * L + threadIdx.x];
    s_alias[threadIdx.x] = al < 0 ? 0 : (al >= L ? L - 1 : al);
    s_alpha[threadIdx.x] = a.alpha[b * L + threadIdx.x];
    s_mask[threadIdx.x] = (float)a.mask[b * L + threadIdx.x];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s_last = srgnn_last(a.mask + b * L, L);
    for (int j = 0; j <= L; ++j) s_start[j] = 0;
    for (int t = 0; t < L; ++t) ++s_start[s_alias[t] + 1];
    for (int j = 0; j < L; ++j) s_start[j + 1] += s_start[j];
    for (int j = 0; j < L; ++j) {                        // positions of node j in ascending order
      int k = s_start[j];
      for (int t = 0; t < L; ++t)
        if (s_alias[t] == j) s_perm[k++] = t;
    }
  }
  const int64_t nb = b * L;
  const f32x4* H = reinterpret_cast<const f32x4*>(a.Hn);
  const f32x4* da = reinterpret_cast<const f32x4*>(a.dcat) + b * 2 * dv;
  for (int t = wave; t < L; t += 4) {
    float d = 0.f;
    const int64_t r = (nb + s_alias[t]) * dv;
    for (int c = lane; c < dv; c += 64) d += dot4(da[c], H[r + c]);
    d = wave_sum(d);
    if (lane == 0) s_dalpha[t] = s_mask[t] * d;
  }
  __syncthreads();
  const int al = s_alias[s_last];
  const f32x4* sig = reinterpret_cast<const f32x4*>(a.sig) + b * L * dv;
  const f32x4* w3 = reinterpret_cast<const f32x4*>(a.w3);
  f32x4* dP = reinterpret_cast<f32x4*>(a.dP);
  f32x4* dH = reinterpret_cast<f32x4*>(a.dH);
  f32x4* dw3p = reinterpret_cast<f32x4*>(a.dw3p) + b * dv;
  const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = threadIdx.x; c < dv; c += blockDim.x) {
    const f32x4 w = w3[c], dac = da[c], dht = da[dv + c];
    f32x4 g1 = z4, gw = z4;
    for (int t = 0; t < L; ++t) {
      const f32x4 s = sig[t * dv + c];
      g1 += (s_dalpha[t] * w) * (s * (1.f - s));
      gw += s_dalpha[t] * s;
    }
    dw3p[c] = gw;
    for (int j = 0; j < L; ++j) {
      f32x4 g2 = z4, gh = z4;
      for (int k = s_start[j]; k < s_start[j + 1]; ++k) {
        const int t = s_perm[k];
        const f32x4 s = sig[t * dv + c];
        g2 += (s_dalpha[t] * w) * (s * (1.f - s));
        gh += (s_alpha[t] * dac) * s_mask[t];
      }
      if (j == al) gh += dht;
      dP[(nb + j) * 2 * dv + c] = j == al ? g1 : z4;
      dP[(nb + j) * 2 * dv + dv + c] = g2;
      dH[(nb + j) * dv + c] = gh;
    }
  }
}

// ---------------------------------------------------------------- pair head (srgnn.py:60-66)
// x_b = <o_b, e[pos_b]> - <o_b, e[neg_b]> into the tail with the 1e-8 outside the log: the query rows o_b are taken from `out`
// (row stride ld_out), both target rows from the table.  One wave per b.
__global__ void __launch_bounds__(256) srgnn_pair_fwd_kernel(const float* __restrict__ out, int64_t ld_out, const float* __restrict__ table,
                                                             int64_t n_table, int D, const int64_t* __restrict__ target, int B,
                                                             float* __restrict__ lossrow, float* __restrict__ coef, int32_t* status) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int dv = D / 4;
  const int64_t ip = checked_id(target[2 * (int64_t)b], n_table, status, lane == 0);
  const int64_t in = checked_id(target[2 * (int64_t)b + 1], n_table, status, lane == 0);
  const f32x4* o = reinterpret_cast<const f32x4*>(out + (int64_t)b * ld_out);
  const f32x4* tp = reinterpret_cast<const f32x4*>(table + ip * D);
  const f32x4* tn = reinterpret_cast<const f32x4*>(table + in * D);
  float sp, sn;
  pair_dots(o, tp, tn, dv, lane, sp, sn);
  if (lane == 0) bpr_tail_log_outside(sp - sn, B, lossrow[b], coef[b]);
}

// dout[b] = c_b (e[pos] - e[neg]) and coef_out[b * coef_stride] = c_b, c_b = coef[b] * grad_scale * (*grad_scale_dev): the
// target rows' gradient (+c_b o_b, -c_b o_b) is left to the occurrence segment sums, which read coef_out.
__global__ void __launch_bounds__(256) srgnn_pair_bwd_kernel(const float* __restrict__ table, int64_t n_table, int D,
                                                             const int64_t* __restrict__ target, const float* __restrict__ coef, int B,
                                                             float gscale, const float* __restrict__ gscale_dev, float* __restrict__ dout,
                                                             int64_t ld_dout, float* __restrict__ coef_out, int64_t coef_stride) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int dv = D / 4;
  const int64_t ip = checked_id(target[2 * (int64_t)b], n_table, nullptr, false);
  const int64_t in = checked_id(target[2 * (int64_t)b + 1], n_table, nullptr, false);
  const float c = coef[b] * gscale * (gscale_dev ? gscale_dev[0] : 1.f);
  const f32x4* tp = reinterpret_cast<const f32x4*>(table + ip * D);
  const f32x4* tn = reinterpret_cast<const f32x4*>(table + in * D);
  f32x4* d = reinterpret_cast<f32x4*>(dout + (int64_t)b * ld_dout);
  for (int k = lane; k < dv; k += 64) d[k] = c * (tp[k] - tn[k]);
  if (lane == 0 && coef_out) coef_out[(int64_t)b * coef_stride] = c;
}

}  // namespace pxr

using namespace pxr;

extern "C" int pxr_srgnn_graph_i64(const int64_t* seq, int64_t B, int L, int64_t n_items, const int64_t* target, int64_t* nodes,
                                   int32_t* alias, float* A, int64_t* occ, int64_t* mask, void* stream) {
  PXR_REQUIRE(seq && nodes && alias && A, "pxr_srgnn_graph_i64: null pointer");
  PXR_REQUIRE(L >= 1 && L <= SRGNN_MAX_L, "pxr_srgnn_graph_i64: need 1 <= L <= %d (L=%d)", SRGNN_MAX_L, L);
  PXR_REQUIRE(B >= 1 && B <= (1ll << 30), "pxr_srgnn_graph_i64: bad batch size %lld", (long long)B);
  PXR_REQUIRE(n_items >= 1 && n_items < (1ll << 31), "pxr_srgnn_graph_i64: need 1 <= n_items < 2^31");
  PXR_REQUIRE(!occ || target, "pxr_srgnn_graph_i64: occ needs target");
  GraphArgs a{};
  a.seq = seq; a.target = target; a.B = B; a.n_items = n_items; a.L = L;
  a.nodes = nodes; a.alias = alias; a.A = A; a.occ = occ; a.mask = mask; a.status = pxr_status_word();
  hipLaunchKernelGGL(srgnn_graph_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
  return pxr_check_launch("pxr_srgnn_graph_i64");
}

extern "C" int pxr_srgnn_prop_f32(const float* A, int B, int L, int D, const float* x, float* y, const float* bias, int transpose,
                                  void* stream) {
  PXR_REQUIRE(A && x && y, "pxr_srgnn_prop_f32: null pointer");
  PXR_REQUIRE((const void*)x != (const void*)y, "pxr_srgnn_prop_f32: x must not alias y");
  PXR_REQUIRE(L >= 1 && L <= SRGNN_MAX_L, "pxr_srgnn_prop_f32: need 1 <= L <= %d (L=%d)", SRGNN_MAX_L, L);
  PXR_REQUIRE(D > 0 && D % 4 == 0 && D <= 2048, "pxr_srgnn_prop_f32: need D %% 4 == 0 and 0 < D <= 2048 (D=%d)", D);
  PXR_REQUIRE(B >= 1, "pxr_srgnn_prop_f32: bad batch size %d", B);
  PXR_REQUIRE(!(transpose && bias), "pxr_srgnn_prop_f32: the transposed product takes no bias");
  PXR_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)bias) & 15) == 0, "pxr_srgnn_prop_f32: operands must be 16-byte aligned");
  hipLaunchKernelGGL(srgnn_prop_kernel, dim3((unsigned)B), dim3(256), (size_t)2 * L * L * sizeof(float), (hipStream_t)stream, A, L,
                     D, x, y, bias, transpose ? 1 : 0);
  return pxr_check_launch("pxr_srgnn_prop_f32");
}

extern "C" int pxr_srgnn_readout_fwd_f32(const float* Hn, const float* P, const int32_t* alias, const int64_t* mask, const float* w3,
                                         int B, int L, int D, float* cat, float* sig, float* alpha, void* stream) {
  PXR_REQUIRE(Hn && P && alias && mask && w3 && cat, "pxr_srgnn_readout_fwd_f32: null pointer");
  PXR_REQUIRE(L >= 1 && L <= SRGNN_MAX_L, "pxr_srgnn_readout_fwd_f32: need 1 <= L <= %d (L=%d)", SRGNN_MAX_L, L);
  PXR_REQUIRE(D > 0 && D % 4 == 0 && D <= 2048, "pxr_srgnn_readout_fwd_f32: need D %% 4 == 0 and 0 < D <= 2048 (D=%d)", D);
  PXR_REQUIRE(B >= 1, "pxr_srgnn_readout_fwd_f32: bad batch size %d", B);
  PXR_REQUIRE((((uintptr_t)Hn | (uintptr_t)P | (uintptr_t)w3 | (uintptr_t)cat | (uintptr_t)sig) & 15) == 0,
              "pxr_srgnn_readout_fwd_f32: operands must be 16-byte aligned");
  ReadoutArgs a{};
  a.Hn = Hn; a.P = P; a.alias = alias; a.mask = mask; a.w3 = w3; a.L = L; a.D = D; a.cat = cat; a.sig = sig; a.alpha = alpha;
  hipLaunchKernelGGL(srgnn_readout_fwd_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
  return pxr_check_launch("pxr_srgnn_readout_fwd_f32");
}

extern "C" int pxr_srgnn_readout_bwd_f32(const float* dcat, const float* Hn, const int32_t* alias, const int64_t* mask,
                                         const float* w3, const float* sig, const float* alpha, int B, int L, int D, float* dP,
                                         float* dH, float* dw3p, void* stream) {
  PXR_REQUIRE(dcat && Hn && alias && mask && w3 && sig && alpha && dP && dH && dw3p, "pxr_srgnn_readout_bwd_f32: null pointer");
  PXR_REQUIRE(L >= 1 && L <= SRGNN_MAX_L, "pxr_srgnn_readout_bwd_f32: need 1 <= L <= %d (L=%d)", SRGNN_MAX_L, L);
  PXR_REQUIRE(D > 0 && D % 4 == 0 && D <= 2048, "pxr_srgnn_readout_bwd_f32: need D %% 4 == 0 and 0 < D <= 2048 (D=%d)", D);
  PXR_REQUIRE(B >= 1, "pxr_srgnn_readout_bwd_f32: bad batch size %d", B);
  PXR_REQUIRE((((uintptr_t)dcat | (uintptr_t)Hn | (uintptr_t)w3 | (uintptr_t)sig | (uintptr_t)dP | (uintptr_t)dH | (uintptr_t)dw3p) &
               15) == 0, "pxr_srgnn_readout_bwd_f32: operands must be 16-byte aligned");
  ReadoutArgs a{};
  a.Hn = Hn; a.alias = alias; a.mask = mask; a.w3 = w3; a.L = L; a.D = D; a.sig = const_cast<float*>(sig);
  a.alpha = const_cast<float*>(alpha); a.dcat = dcat; a.dP = dP; a.dH = dH; a.dw3p = dw3p;
  hipLaunchKernelGGL(srgnn_readout_bwd_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
  return pxr_check_launch("pxr_srgnn_readout_bwd_f32");
}

extern "C" int pxr_srgnn_pair_fwd_f32(const float* out, int64_t ld_out, const float* table, int64_t n_table, int D,
                                      const int64_t* target, int B, float* lossrow, float* coef, float* loss, void* stream) {
  PXR_REQUIRE(out && table && target && lossrow && coef && loss, "pxr_srgnn_pair_fwd_f32: null pointer");
  PXR_REQUIRE(n_table > 0, "pxr_srgnn_pair_fwd_f32: empty table");
  PXR_REQUIRE(D > 0 && D % 4 == 0 && ld_out >= D && ld_out % 4 == 0, "pxr_srgnn_pair_fwd_f32: need D %% 4 == 0, ld_out >= D");
  PXR_REQUIRE(B > 0 && B <= (1 << 28), "pxr_srgnn_pair_fwd_f32: bad batch size %d", B);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(srgnn_pair_fwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, out, ld_out, table, n_table, D, target,
                     B, lossrow, coef, pxr_status_word());
  const int rc = pxr_check_launch("pxr_srgnn_pair_fwd_f32");
  if (rc) return rc;
  return pxr_bpr_loss_reduce(lossrow, B, 1, loss, stream);        // loss = (1/B) sum_b lossrow[b], fixed order
}

extern "C" int pxr_srgnn_pair_bwd_f32(const float* table, int64_t n_table, int D, const int64_t* target, const float* coef, int B,
                                      float grad_scale, const float* grad_scale_dev, float* dout, int64_t ld_dout, float* coef_out,
                                      int64_t coef_stride, void* stream) {
  PXR_REQUIRE(table && target && coef && dout, "pxr_srgnn_pair_bwd_f32: null pointer");
  PXR_REQUIRE(n_table > 0, "pxr_srgnn_pair_bwd_f32: empty table");
  PXR_REQUIRE(D > 0 && D % 4 == 0 && ld_dout >= D && ld_dout % 4 == 0, "pxr_srgnn_pair_bwd_f32: need D %% 4 == 0, ld_dout >= D");
  PXR_REQUIRE(B > 0 && B <= (1 << 28), "pxr_srgnn_pair_bwd_f32: bad batch size %d", B);
  hipLaunchKernelGGL(srgnn_pair_bwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, table, n_table, D,
                     target, coef, B, grad_scale, grad_scale_dev, dout, ld_dout, coef_out, coef_stride);
  return pxr_check_launch("pxr_srgnn_pair_bwd_f32");
}
