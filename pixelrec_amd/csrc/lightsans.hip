// lightsans.hip -- the low-rank interest attention of LightSANs (reference code/REC/model/layers.py:762-932:
// ItemToInterestAggregation, LightMultiHeadAttention) between the fused q|k|v projection and the `dense` projection.  The
// GEMMs, LayerNorms, FFN and loss head around it are the library's; nothing here uses float atomics or scratch, and every
// sum runs in a fixed order, so every output is bit-identical from run to run.
//
// Per sequence b (L positions, width D = H heads x dh, K interests), with q, k, v the rows of the q|k|v projection:
//   pi_K = softmax over l of (k thK) [L, K],  Kp = pi_K^T k [K, D];  pi_V, Vp likewise from v and thV    (theta [D, K])
//   per head h:  S = q_h Kp_h^T / sqrt(dh) [L, K],  P = softmax over the L QUERIES (dim -2),  P~ = dropout(P)
//                ctx_h = P~ Vp_h + A_h v_h          A [H, L, L]: the position probabilities (batch-independent)
//   A_h = softmax over the queries i of ((pq_h pos_scaling) pk_h^T / sqrt(dh)), pos_scaling = (2 dh)^-1/2
// No mask anywhere: padded positions are ordinary rows.  Because P and A are normalised over queries, every position reads
// every other one, so the whole [L, D] slab of each sequence is needed even when only the last position is scored.
#include "pxr_common.h"

namespace pxr {

constexpr int LS_MAX_L = 64, LS_MAX_D = 1024, LS_MAX_K = 16, LS_T = 256, LS_NW = LS_T / 64;

__device__ __forceinline__ float ls_dot4(const float* __restrict__ a, const float* __restrict__ b, int n) {
  // sum_c a[c] b[c], n % 4 == 0, both 16-byte aligned; fixed order (four lanes of partials, then ((0 + 1) + (2 + 3)))
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = 0; c < n; c += 4) {
    const float4 x = *reinterpret_cast<const float4*>(a + c), y = *reinterpret_cast<const float4*>(b + c);
    s.x += x.x * y.x; s.y += x.y * y.y; s.z += x.z * y.z; s.w += x.w * y.w;
  }
  return (s.x + s.y) + (s.z + s.w);
}

struct CoreArgs {
  const float* qkv;        // [B*L, 3D]
  const float* th;         // [2, D, K]: thK then thV
  const float* A;          // [H, L, L]
  int L, D, H, K;
  float p_drop, inv_keep, inv_sqrt_dh;
  uint32_t thr, stream;
  uint64_t seed;
  const int64_t* step_dev;
  // forward
  float* ctx;              // [B*L, D]
  float* pi;               // [B, 2, L, K] or NULL (the interest softmaxes)
  float* probs;            // [B, H, L, K] or NULL (P before dropout)
  float* KVp;              // [B, 2K, D]: Kp rows then Vp rows
  // backward
  const float* dctx;       // [B*L, D]
  float* dqkv;             // [B*L, 3D]
  float* dKVp;             // [B, 2K, D]
  float* dth;              // [B, 2 D K]: per-sequence parts of d thK | d thV
  float* dA;               // [B, H L L]: per-sequence parts of d A
};

// logits of both poolings, one wave per (tensor, row): lanes stride over d, K partials per lane, then one wave sum per interest
__device__ __forceinline__ void ls_interest_softmax(const CoreArgs& a, int64_t b, float (*sPi)[LS_MAX_L][LS_MAX_K], int lane, int wave) {
  const int L = a.L, D = a.D, K = a.K;
  for (int r = wave; r < 2 * L; r += LS_NW) {
    const int which = r / L, l = r - which * L;
    const float* x = a.qkv + (b * L + l) * 3 * D + (int64_t)(1 + which) * D;
    const float* th = a.th + (int64_t)which * D * K;
    float acc[LS_MAX_K];
#pragma unroll
    for (int k = 0; k < LS_MAX_K; ++k) acc[k] = 0.f;
    for (int d = lane; d < D; d += 64) {
      const float xv = x[d];
#pragma unroll
      for (int k = 0; k < LS_MAX_K; ++k)
        if (k < K) acc[k] += xv * th[(int64_t)d * K + k];
    }
#pragma unroll
    for (int k = 0; k < LS_MAX_K; ++k)
      if (k < K) {
        const float s = wave_sum(acc[k]);
        if (lane == 0) sPi[which][l][k] = s;
      }
  }
  __syncthreads();
  // softmax over l of each (tensor, interest) column, one thread per column
  if ((int)threadIdx.x < 2 * K) {
    const int which = threadIdx.x / K, k = threadIdx.x - which * K;
    float m = -INFINITY;
    for (int l = 0; l < L; ++l) m = fmaxf(m, sPi[which][l][k]);
    float sum = 0.f;
    for (int l = 0; l < L; ++l) {
      const float e = expf(sPi[which][l][k] - m);
      sPi[which][l][k] = e;
      sum += e;
    }
    for (int l = 0; l < L; ++l) {
      const float p = sPi[which][l][k] / sum;
      sPi[which][l][k] = p;
      if (a.pi) a.pi[((b * 2 + which) * L + l) * K + k] = p;
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(LS_T) lightsans_fwd_kernel(CoreArgs a) {
  __shared__ float sPi[2][LS_MAX_L][LS_MAX_K];
  __shared__ float sA[LS_MAX_L * LS_MAX_L];
  __shared__ float sS[LS_MAX_L][LS_MAX_K];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int L = a.L, D = a.D, H = a.H, K = a.K, dh = D / H;
  const uint64_t seed = a.seed + (a.step_dev ? (uint64_t)a.step_dev[0] : 0ull);
  ls_interest_softmax(a, b, sPi, lane, wave);

  // pooled interests: Kp[k, d] = sum_l pi_K[l, k] k[l, d] (and Vp), one thread per column d
  float* KVp = a.KVp + b * 2 * K * D;
  for (int d = threadIdx.x; d < D; d += LS_T)
    for (int which = 0; which < 2; ++which) {
      float acc[LS_MAX_K];
#pragma unroll
      for (int k = 0; k < LS_MAX_K; ++k) acc[k] = 0.f;
      for (int l = 0; l < L; ++l) {
        const float xv = a.qkv[(b * L + l) * 3 * D + (int64_t)(1 + which) * D + d];
#pragma unroll
        for (int k = 0; k < LS_MAX_K; ++k)
          if (k < K) acc[k] += sPi[which][l][k] * xv;
      }
#pragma unroll
      for (int k = 0; k < LS_MAX_K; ++k)
        if (k < K) KVp[(int64_t)(which * K + k) * D + d] = acc[k];
    }
  __syncthreads();          // (KVp is read back by other threads of this workgroup below)

  for (int h = 0; h < H; ++h) {
    const int c0 = h * dh;
    for (int f = threadIdx.x; f < L * L; f += LS_T) sA[f] = a.A[(int64_t)h * L * L + f];
    // S[i, k] = q_h[i] . Kp_h[k] / sqrt(dh): one wave per query row
    for (int i = wave; i < L; i += LS_NW) {
      const float* q = a.qkv + (b * L + i) * 3 * D + c0;
      float acc[LS_MAX_K];
#pragma unroll
      for (int k = 0; k < LS_MAX_K; ++k) acc[k] = 0.f;
      for (int c = lane; c < dh; c += 64) {
        const float qv = q[c];
#pragma unroll
        for (int k = 0; k < LS_MAX_K; ++k)
          if (k < K) acc[k] += qv * KVp[(int64_t)k * D + c0 + c];
      }
#pragma unroll
      for (int k = 0; k < LS_MAX_K; ++k)
        if (k < K) {
          const float s = wave_sum(acc[k]);
          if (lane == 0) sS[i][k] = s * a.inv_sqrt_dh;
        }
    }
    __syncthreads();
    // softmax over the queries i of each interest column; P saved before dropout, P~ kept in LDS
    if ((int)threadIdx.x < K) {
      const int k = threadIdx.x;
      float m = -INFINITY;
      for (int i = 0; i < L; ++i) m = fmaxf(m, sS[i][k]);
      float sum = 0.f;
      for (int i = 0; i < L; ++i) {
        const float e = expf(sS[i][k] - m);
        sS[i][k] = e;
        sum += e;
      }
      for (int i = 0; i < L; ++i) {
        const float p = sS[i][k] / sum;
        const int64_t pi = ((b * H + h) * L + i) * K + k;
        if (a.probs) a.probs[pi] = p;
        sS[i][k] = (a.thr != 0u) ? (pxr_keep(seed, a.stream, (uint64_t)pi, a.thr) ? p * a.inv_keep : 0.f) : p;
      }
    }
    __syncthreads();
    // ctx[i, c] = sum_k P~[i, k] Vp[k, c] + sum_j A_h[i, j] v[j, c]
    for (int f = threadIdx.x; f < L * dh; f += LS_T) {
      const int i = f / dh, c = c0 + (f - (f / dh) * dh);
      float ci = 0.f, cp = 0.f;
      for (int k = 0; k < K; ++k) ci += sS[i][k] * KVp[(int64_t)(K + k) * D + c];
      for (int j = 0; j < L; ++j) cp += sA[i * L + j] * a.qkv[(b * L + j) * 3 * D + 2 * D + c];
      a.ctx[(b * L + i) * D + c] = ci + cp;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(LS_T) lightsans_bwd_kernel(CoreArgs a) {
  __shared__ float sPi[2][LS_MAX_L][LS_MAX_K];    // interest softmaxes
  __shared__ float sdPi[2][LS_MAX_L][LS_MAX_K];   // d pi, summed over the heads in ascending order; then d logits
  __shared__ float sA[LS_MAX_L * LS_MAX_L];
  __shared__ float sP[LS_MAX_L][LS_MAX_K];        // P before dropout
  __shared__ float sPd[LS_MAX_L][LS_MAX_K];       // P~
  __shared__ float sdS[LS_MAX_L][LS_MAX_K];       // d P~, then d S / sqrt(dh)
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int L = a.L, D = a.D, H = a.H, K = a.K, dh = D / H;
  const int64_t ld = 3 * (int64_t)D;
  const uint64_t seed = a.seed + (a.step_dev ? (uint64_t)a.step_dev[0] : 0ull);
  const bool drop = a.thr != 0u;
  const float* KVp = a.KVp + b * 2 * K * D;
  float* dKVp = a.dKVp + b * 2 * K * D;
  const float* dC = a.dctx + b * L * D;
  const float* X = a.qkv + b * L * ld;
  float* dX = a.dqkv + b * L * ld;
  for (int f = threadIdx.x; f < 2 * LS_MAX_L * LS_MAX_K; f += LS_T) {
    const int which = f / (LS_MAX_L * LS_MAX_K), r = f - which * LS_MAX_L * LS_MAX_K, l = r / LS_MAX_K, k = r - l * LS_MAX_K;
    sPi[which][l][k] = (l < L && k < K) ? a.pi[((b * 2 + which) * L + l) * K + k] : 0.f;
    sdPi[which][l][k] = 0.f;
  }

  for (int h = 0; h < H; ++h) {
    const int c0 = h * dh;
    for (int f = threadIdx.x; f < L * L; f += LS_T) sA[f] = a.A[(int64_t)h * L * L + f];
    for (int f = threadIdx.x; f < L * K; f += LS_T) {
      const int i = f / K, k = f - i * K;
      const int64_t pi = ((b * H + h) * L + i) * K + k;
      const float p = a.probs[pi];
      sP[i][k] = p;
      sPd[i][k] = drop ? (pxr_keep(seed, a.stream, (uint64_t)pi, a.thr) ? p * a.inv_keep : 0.f) : p;
    }
    // d P~[i, k] = dctx_h[i] . Vp_h[k]: one wave per query row
    for (int i = wave; i < L; i += LS_NW) {
      float acc[LS_MAX_K];
#pragma unroll
      for (int k = 0; k < LS_MAX_K; ++k) acc[k] = 0.f;
      for (int c = lane; c < dh; c += 64) {
        const float g = dC[(int64_t)i * D + c0 + c];
#pragma unroll
        for (int k = 0; k < LS_MAX_K; ++k)
          if (k < K) acc[k] += g * KVp[(int64_t)(K + k) * D + c0 + c];
      }
#pragma unroll
      for (int k = 0; k < LS_MAX_K; ++k)
        if (k < K) {
          const float s = wave_sum(acc[k]);
          if (lane == 0) sdS[i][k] = s;
        }
    }
    __syncthreads();
    // through the dropout and the softmax over the queries: dS = P (dP - sum_i P dP), scaled by 1/sqrt(dh)
    if ((int)threadIdx.x < K) {
      const int k = threadIdx.x;
      for (int i = 0; i < L; ++i) {
        const int64_t pi = ((b * H + h) * L + i) * K + k;
        if (drop) sdS[i][k] = pxr_keep(seed, a.stream, (uint64_t)pi, a.thr) ? sdS[i][k] * a.inv_keep : 0.f;
      }
      float dot = 0.f;
      for (int i = 0; i < L; ++i) dot += sP[i][k] * sdS[i][k];
      for (int i = 0; i < L; ++i) sdS[i][k] = sP[i][k] * (sdS[i][k] - dot) * a.inv_sqrt_dh;
    }
    __syncthreads();
    // per column c of the head: d Kp, d Vp, d q, and the positional path into v (kept in the v slot of dqkv until the end)
    for (int c = c0 + threadIdx.x; c < c0 + dh; c += LS_T) {
      float kp[LS_MAX_K], dk[LS_MAX_K], dv[LS_MAX_K];
#pragma unroll
      for (int k = 0; k < LS_MAX_K; ++k) {
        kp[k] = (k < K) ? KVp[(int64_t)k * D + c] : 0.f;
        dk[k] = dv[k] = 0.f;
      }
      for (int i = 0; i < L; ++i) {
        const float qv = X[(int64_t)i * ld + c], g = dC[(int64_t)i * D + c];
        float dq = 0.f;
#pragma unroll
        for (int k = 0; k < LS_MAX_K; ++k)
          if (k < K) {
            dk[k] += sdS[i][k] * qv;
            dv[k] += sPd[i][k] * g;
            dq += sdS[i][k] * kp[k];
          }
        dX[(int64_t)i * ld + c] = dq;
      }
#pragma unroll
      for (int k = 0; k < LS_MAX_K; ++k)
        if (k < K) {
          dKVp[(int64_t)k * D + c] = dk[k];
          dKVp[(int64_t)(K + k) * D + c] = dv[k];
        }
      for (int j = 0; j < L; ++j) {
        float s = 0.f;
        for (int i = 0; i < L; ++i) s += sA[i * L + j] * dC[(int64_t)i * D + c];
        dX[(int64_t)j * ld + 2 * D + c] = s;
      }
    }
    // d A_h[i, j] = dctx_h[i] . v_h[j]: one wave per pair
    for (int p = wave; p < L * L; p += LS_NW) {
      const int i = p / L, j = p - i * L;
      float s = 0.f;
      for (int c = lane; c < dh; c += 64) s += dC[(int64_t)i * D + c0 + c] * X[(int64_t)j * ld + 2 * D + c0 + c];
      s = wave_sum(s);
      if (lane == 0) a.dA[((b * H + h) * L + i) * L + j] = s;
    }
    __syncthreads();          // (this head's d Kp / d Vp columns are read back below)
    // d pi[l, k] += d Kp_h[k] . k_h[l]  (and d Vp_h . v_h): one wave per (tensor, row)
    for (int r = wave; r < 2 * L; r += LS_NW) {
      const int which = r / L, l = r - which * L;
      float acc[LS_MAX_K];
#pragma unroll
      for (int k = 0; k < LS_MAX_K; ++k) acc[k] = 0.f;
      for (int c = lane; c < dh; c += 64) {
        const float xv = X[(int64_t)l * ld + (int64_t)(1 + which) * D + c0 + c];
#pragma unroll
        for (int k = 0; k < LS_MAX_K; ++k)
          if (k < K) acc[k] += xv * dKVp[(int64_t)(which * K + k) * D + c0 + c];
      }
#pragma unroll
      for (int k = 0; k < LS_MAX_K; ++k)
        if (k < K) {
          const float s = wave_sum(acc[k]);
          if (lane == 0) sdPi[which][l][k] += s;
        }
    }
    __syncthreads();
  }

  // through the interest softmaxes over l: d logits = pi (d pi - sum_l pi d pi)
  if ((int)threadIdx.x < 2 * K) {
    const int which = threadIdx.x / K, k = threadIdx.x - which * K;
    float dot = 0.f;
    for (int l = 0; l < L; ++l) dot += sPi[which][l][k] * sdPi[which][l][k];
    for (int l = 0; l < L; ++l) sdPi[which][l][k] = sPi[which][l][k] * (sdPi[which][l][k] - dot);
  }
  __syncthreads();
  // d k[l, d] = sum_k pi_K[l, k] d Kp[k, d] + sum_k dlogit_K[l, k] thK[d, k]; d v likewise plus its positional path;
  // d theta parts [d, k] = sum_l x[l, d] dlogit[l, k]
  for (int d = threadIdx.x; d < D; d += LS_T)
    for (int which = 0; which < 2; ++which) {
      const float* th = a.th + (int64_t)which * D * K + (int64_t)d * K;
      float g[LS_MAX_K], t[LS_MAX_K], dt[LS_MAX_K];
#pragma unroll
      for (int k = 0; k < LS_MAX_K; ++k) {
        g[k] = (k < K) ? dKVp[(int64_t)(which * K + k) * D + d] : 0.f;
        t[k] = (k < K) ? th[k] : 0.f;
        dt[k] = 0.f;
      }
      const int64_t col = (int64_t)(1 + which) * D + d;
      for (int l = 0; l < L; ++l) {
        float pooled = 0.f, logit = 0.f;
        const float xv = X[(int64_t)l * ld + col];
#pragma unroll
        for (int k = 0; k < LS_MAX_K; ++k)
          if (k < K) {
            pooled += sPi[which][l][k] * g[k];
            logit += sdPi[which][l][k] * t[k];
            dt[k] += xv * sdPi[which][l][k];
          }
        float r = pooled + logit;
        if (which == 1) r += dX[(int64_t)l * ld + col];        // the positional path, written per head above
        dX[(int64_t)l * ld + col] = r;
      }
      float* out = a.dth + b * 2 * D * K + (int64_t)which * D * K + (int64_t)d * K;
#pragma unroll
      for (int k = 0; k < LS_MAX_K; ++k)
        if (k < K) out[k] = dt[k];
    }
}

// ---------------------------------------------------------------- position probabilities: one workgroup per head
__global__ void __launch_bounds__(LS_T) lightsans_pos_fwd_kernel(const float* __restrict__ pqk, int L, int D, int H, float scale,
                                                                  float* __restrict__ A) {
  __shared__ float sS[LS_MAX_L * LS_MAX_L];
  const int h = blockIdx.x, dh = D / H;
  for (int p = threadIdx.x; p < L * L; p += LS_T) {
    const int i = p / L, j = p - i * L;
    sS[p] = ls_dot4(pqk + (int64_t)i * 2 * D + h * dh, pqk + (int64_t)j * 2 * D + D + h * dh, dh) * scale;
  }
  __syncthreads();
  if ((int)threadIdx.x < L) {            // softmax over the queries i of column j
    const int j = threadIdx.x;
    float m = -INFINITY;
    for (int i = 0; i < L; ++i) m = fmaxf(m, sS[i * L + j]);
    float sum = 0.f;
    for (int i = 0; i < L; ++i) {
      const float e = expf(sS[i * L + j] - m);
      sS[i * L + j] = e;
      sum += e;
    }
    for (int i = 0; i < L; ++i) A[((int64_t)h * L + i) * L + j] = sS[i * L + j] / sum;
  }
}

__global__ void __launch_bounds__(LS_T) lightsans_pos_bwd_kernel(const float* __restrict__ pqk, const float* __restrict__ A,
                                                                  const float* __restrict__ dA, int L, int D, int H, float scale,
                                                                  float* __restrict__ dpqk) {
  __shared__ float sG[LS_MAX_L * LS_MAX_L];
  const int h = blockIdx.x, dh = D / H;
  const float* Ah = A + (int64_t)h * L * L;
  const float* dAh = dA + (int64_t)h * L * L;
  if ((int)threadIdx.x < L) {            // d scores = A (dA - sum_i A dA) per column j, times the score scale
    const int j = threadIdx.x;
    float dot = 0.f;
    for (int i = 0; i < L; ++i) dot += Ah[i * L + j] * dAh[i * L + j];
    for (int i = 0; i < L; ++i) sG[i * L + j] = Ah[i * L + j] * (dAh[i * L + j] - dot) * scale;
  }
  __syncthreads();
  for (int f = threadIdx.x; f < 2 * L * dh; f += LS_T) {
    const int which = f / (L * dh), r = f - which * L * dh, i = r / dh, c = h * dh + (r - (r / dh) * dh);
    float s = 0.f;
    if (which == 0)                      // d pq[i] = sum_j G[i, j] pk[j]
      for (int j = 0; j < L; ++j) s += sG[i * L + j] * pqk[(int64_t)j * 2 * D + D + c];
    else                                 // d pk[i] = sum_q G[q, i] pq[q]
      for (int q = 0; q < L; ++q) s += sG[q * L + i] * pqk[(int64_t)q * 2 * D + c];
    dpqk[(int64_t)i * 2 * D + (int64_t)which * D + c] = s;
  }
}

}  // namespace pxr

using namespace pxr;

static int ls_check_shape(const char* what, int B, int L, int D, int H, int K) {
  PXR_REQUIRE(L >= 1 && L <= LS_MAX_L, "%s: need 1 <= L <= %d (L=%d)", what, LS_MAX_L, L);
  PXR_REQUIRE(H >= 1 && D >= 4 && D <= LS_MAX_D && D % (4 * H) == 0, "%s: need D <= %d and D %% (4 H) == 0 (D=%d, H=%d)", what,
              LS_MAX_D, D, H);
  PXR_REQUIRE(K >= 1 && K <= LS_MAX_K, "%s: need 1 <= K <= %d (K=%d)", what, LS_MAX_K, K);
  PXR_REQUIRE(B >= 1 && B <= (1 << 24), "%s: bad batch size %d", what, B);
  return PXR_OK;
}

static float ls_inv_keep(float p) { return p > 0.f ? 1.0f / (1.0f - p) : 1.0f; }

extern "C" int pxr_lightsans_fwd_f32(const float* qkv, const float* theta, const float* A, int B, int L, int D, int H, int K,
                                     float p_drop, uint64_t seed, uint32_t stream_id, const int64_t* step_dev, float* ctx, float* pi,
                                     float* probs, float* KVp, void* stream) {
  PXR_REQUIRE(qkv && theta && A && ctx && KVp, "pxr_lightsans_fwd_f32: null pointer");
  PXR_REQUIRE((pi == nullptr) == (probs == nullptr), "pxr_lightsans_fwd_f32: pi and probs are saved together or not at all");
  if (int rc = ls_check_shape("pxr_lightsans_fwd_f32", B, L, D, H, K)) return rc;
  PXR_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "pxr_lightsans_fwd_f32: need 0 <= p_drop < 1 (p=%g)", (double)p_drop);
  CoreArgs a{};
  a.qkv = qkv; a.th = theta; a.A = A; a.L = L; a.D = D; a.H = H; a.K = K;
  a.p_drop = p_drop; a.inv_keep = ls_inv_keep(p_drop); a.inv_sqrt_dh = 1.0f / sqrtf((float)(D / H));
  a.thr = pxr_drop_threshold(p_drop); a.stream = stream_id; a.seed = seed; a.step_dev = step_dev;
  a.ctx = ctx; a.pi = pi; a.probs = probs; a.KVp = KVp;
  hipLaunchKernelGGL(lightsans_fwd_kernel, dim3((unsigned)B), dim3(LS_T), 0, (hipStream_t)stream, a);
  return pxr_check_launch("pxr_lightsans_fwd_f32");
}

extern "C" int pxr_lightsans_bwd_f32(const float* dctx, const float* qkv, const float* theta, const float* A, const float* pi,
                                     const float* probs, const float* KVp, int B, int L, int D, int H, int K, float p_drop, uint64_t seed,
                                     uint32_t stream_id, const int64_t* step_dev, float* dqkv, float* dKVp, float* dtheta_part,
                                     float* dA_part, void* stream) {
  PXR_REQUIRE(dctx && qkv && theta && A && pi && probs && KVp && dqkv && dKVp && dtheta_part && dA_part,
              "pxr_lightsans_bwd_f32: null pointer");
  if (int rc = ls_check_shape("pxr_lightsans_bwd_f32", B, L, D, H, K)) return rc;
  PXR_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "pxr_lightsans_bwd_f32: need 0 <= p_drop < 1 (p=%g)", (double)p_drop);
  PXR_REQUIRE((const void*)dqkv != (const void*)qkv, "pxr_lightsans_bwd_f32: dqkv must not alias qkv");
  CoreArgs a{};
  a.qkv = qkv; a.th = theta; a.A = A; a.L = L; a.D = D; a.H = H; a.K = K;
  a.p_drop = p_drop; a.inv_keep = ls_inv_keep(p_drop); a.inv_sqrt_dh = 1.0f / sqrtf((float)(D / H));
  a.thr = pxr_drop_threshold(p_drop); a.stream = stream_id; a.seed = seed; a.step_dev = step_dev;
  a.pi = const_cast<float*>(pi); a.probs = const_cast<float*>(probs); a.KVp = const_cast<float*>(KVp);
  a.dctx = dctx; a.dqkv = dqkv; a.dKVp = dKVp; a.dth = dtheta_part; a.dA = dA_part;
  hipLaunchKernelGGL(lightsans_bwd_kernel, dim3((unsigned)B), dim3(LS_T), 0, (hipStream_t)stream, a);
  return pxr_check_launch("pxr_lightsans_bwd_f32");
}

static float ls_pos_scale(int D, int H) {
  const float dh = (float)(D / H);
  return (1.0f / sqrtf(2.0f * dh)) / sqrtf(dh);        // pos_scaling, then the division by sqrt(dh) (layers.py:829,866-867)
}

extern "C" int pxr_lightsans_pos_fwd_f32(const float* pqk, int L, int D, int H, float* A, void* stream) {
  PXR_REQUIRE(pqk && A, "pxr_lightsans_pos_fwd_f32: null pointer");
  if (int rc = ls_check_shape("pxr_lightsans_pos_fwd_f32", 1, L, D, H, 1)) return rc;
  // (the score dot products read pqk as float4: rows 2D floats apart and head offsets are multiples of 4 floats, so an aligned
  // base keeps every access aligned)
  PXR_REQUIRE(((uintptr_t)pqk & 15) == 0, "pxr_lightsans_pos_fwd_f32: pqk must be 16-byte aligned");
  hipLaunchKernelGGL(lightsans_pos_fwd_kernel, dim3((unsigned)H), dim3(LS_T), 0, (hipStream_t)stream, pqk, L, D, H, ls_pos_scale(D, H),
                     A);
  return pxr_check_launch("pxr_lightsans_pos_fwd_f32");
}

extern "C" int pxr_lightsans_pos_bwd_f32(const float* pqk, const float* A, const float* dA, int L, int D, int H, float* dpqk,
                                         void* stream) {
  PXR_REQUIRE(pqk && A && dA && dpqk, "pxr_lightsans_pos_bwd_f32: null pointer");
  if (int rc = ls_check_shape("pxr_lightsans_pos_bwd_f32", 1, L, D, H, 1)) return rc;
  hipLaunchKernelGGL(lightsans_pos_bwd_kernel, dim3((unsigned)H), dim3(LS_T), 0, (hipStream_t)stream, pqk, A, dA, L, D, H,
                     ls_pos_scale(D, H), dpqk);
  return pxr_check_launch("pxr_lightsans_pos_bwd_f32");
}
