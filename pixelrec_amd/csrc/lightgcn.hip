// lightgcn.hip -- LightGCN (reference code/REC/model/IDNet/lightgcn.py, layers.py:13-22): the graph propagation as a CSR SpMM
// with a fused layer-mean epilogue, and the pair loss head (forward and a deterministic scatter of its gradient rows).
//
// Graph: rows of A are nodes (users 0..U-1, then items U..U+I-1), A[i,j] = w_ij = d_i^-1/2 d_j^-1/2 for every training edge,
// both directions, duplicates kept (dataload.py:318-339).  A is symmetric, so one CSR serves the forward y = A x (PyG's
// source -> target add-aggregation) and the backward, which is the same product applied to the gradient.
//
// SpMM layout: one wave per row.  A row of D floats is D/4 16-byte chunks; a wave is cut into P = 64/G groups of G lanes
// (G = the next power of two >= D/4, at most 64), each group gathers a different neighbour row, and every lane issues U
// neighbour loads before the first add, so U*P rows are in flight per wave (the gather is latency bound: the table is larger
// than the Infinity Cache at the Pixel200K shape).  D > 256: G = 64 and CH = D/256 chunks per lane.  Rows of more than
// `part_len` edges (Zipf-popular items: tens of thousands) are cut into parts that go to waves of their own and are summed in
// part order by a second launch -- the fixed-order idea of the split segment sums in embed_grad.hip.  No float atomics anywhere:
// every output is bit-identical from run to run.
#include "pair_head.cuh"

namespace pxr {

struct SpmmArgs {
  const int64_t* row_ptr;
  const int32_t* col;
  const float* w;
  int64_t n_rows;
  int dv, lg;                 // D / 4; log2 of the lanes per group
  const int32_t* split_row;   // [n_split] rows of more than part_len edges
  const int32_t* split_part0; // [n_split + 1] first part of each split row
  const int32_t* part_owner;  // [n_parts] split-row index of each part
  int n_split, n_parts, part_len;
  const f32x4* x;
  f32x4* y;
  const f32x4* acc_in;
  f32x4* acc_out;
  float scale;
  f32x4* ws;                  // [n_parts, dv] part sums
  int32_t* status;
};

// out chunk c of row r: y = s; acc_out = (acc_in + s) * scale
__device__ __forceinline__ void spmm_store(const SpmmArgs& a, int64_t r, int c, const f32x4& s) {
  const int64_t o = r * a.dv + c;
  if (a.y) a.y[o] = s;
  if (a.acc_out) a.acc_out[o] = (a.acc_in ? a.acc_in[o] + s : s) * a.scale;
}

template <int CH>
__global__ void __launch_bounds__(256) lgcn_spmm_kernel(SpmmArgs a) {
  constexpr int U = CH == 1 ? 8 : (CH == 2 ? 4 : (CH == 4 ? 2 : 1));
  const int lane = threadIdx.x & 63;
  const int64_t gw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int G = 1 << a.lg, P = 64 >> a.lg, p = lane >> a.lg, gl = lane & (G - 1);
  // the parts of long rows come first in the grid: the longest waves start earliest instead of forming the tail
  int64_t r, b, e, q = -1;
  if (gw >= a.n_parts) {
    r = gw - a.n_parts;
    if (r >= a.n_rows) return;
    b = a.row_ptr[r];
    e = a.row_ptr[r + 1];
    if (e - b > a.part_len) return;               // a split row: its parts are summed by their own waves
  } else {
    q = gw;
    const int j = a.part_owner[q];
    if (j < 0 || j >= a.n_split) return;
    r = a.split_row[j];
    if (r < 0 || r >= a.n_rows) return;
    const int64_t k = q - a.split_part0[j];
    const int64_t rb = a.row_ptr[r], re = a.row_ptr[r + 1];
    b = rb + k * a.part_len;
    e = b + a.part_len < re ? b + a.part_len : re;
  }
  f32x4 s[CH];
#pragma unroll
  for (int h = 0; h < CH; ++h) s[h] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t base = b; base < e; base += (int64_t)U * P) {
    int64_t cj[U];
    float wj[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ed = base + (int64_t)u * P + p;
      cj[u] = -1;
      wj[u] = 0.f;
      if (ed < e) {
        cj[u] = checked_id(a.col[ed], a.n_rows, a.status, gl == 0);     // a neighbour outside the table: flagged, clamped
        wj[u] = a.w[ed];
      }
    }
    f32x4 v[U][CH];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int h = 0; h < CH; ++h) {
        const int c = gl + h * 64;
        v[u][h] = (cj[u] >= 0 && c < a.dv) ? a.x[cj[u] * a.dv + c] : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int h = 0; h < CH; ++h) s[h] += wj[u] * v[u][h];
  }
  // the P groups hold partial sums of the same chunks: a butterfly in a fixed order
  for (int off = G; off < 64; off <<= 1)
#pragma unroll
    for (int h = 0; h < CH; ++h) {
      s[h].x += __shfl_xor(s[h].x, off);
      s[h].y += __shfl_xor(s[h].y, off);
      s[h].z += __shfl_xor(s[h].z, off);
      s[h].w += __shfl_xor(s[h].w, off);
    }
  if (p != 0) return;
#pragma unroll
  for (int h = 0; h < CH; ++h) {
    const int c = gl + h * 64;
    if (c >= a.dv) continue;
    if (q >= 0) a.ws[q * a.dv + c] = s[h];
    else spmm_store(a, r, c, s[h]);
  }
}

// one wave per split row: its part sums in part order, then the epilogue
__global__ void __launch_bounds__(256) lgcn_spmm_combine_kernel(SpmmArgs a) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= a.n_split) return;
  const int64_t r = a.split_row[j];
  if (r < 0 || r >= a.n_rows) return;
  const int p0 = a.split_part0[j], p1 = a.split_part0[j + 1];
  for (int c = lane; c < a.dv; c += 64) {
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
    int k = p0;
    for (; k + 4 <= p1; k += 4) {                 // four loads in flight, added in part order
      f32x4 t[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) t[u] = a.ws[(int64_t)(k + u) * a.dv + c];
#pragma unroll
      for (int u = 0; u < 4; ++u) s += t[u];
    }
    for (; k < p1; ++k) s += a.ws[(int64_t)k * a.dv + c];
    spmm_store(a, r, c, s);
  }
}

// ---------------------------------------------------------------- pair head (lightgcn.py:70-78)
// x_b = <u_b, i+_b> - <u_b, i-_b> into the tail with the 1e-8 outside the log.  One wave per b.
struct PairArgs {
  const f32x4* emb;           // E_final [n_users + n_items, dv]
  int64_t n_users, n_items;
  int dv, B;
  const int64_t* user;        // [B]
  const int64_t* item;        // [B, 2] = (positive, negative)
  float* diff;                // [B] x_b
  float* coef;                // [B] d loss / d x_b
  float* lossrow;             // [B]
  int32_t* nodes;             // [3B] (user node, positive node, negative node) per b
  int32_t* status;
};

__global__ void __launch_bounds__(256) lgcn_pair_fwd_kernel(PairArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const int64_t nu = checked_id(a.user[b], a.n_users, a.status, lane == 0);
  const int64_t np = a.n_users + checked_id(a.item[2 * (int64_t)b], a.n_items, a.status, lane == 0);
  const int64_t nn = a.n_users + checked_id(a.item[2 * (int64_t)b + 1], a.n_items, a.status, lane == 0);
  float sp, sn;
  pair_dots(a.emb + nu * a.dv, a.emb + np * a.dv, a.emb + nn * a.dv, a.dv, lane, sp, sn);
  if (lane != 0) return;
  a.diff[b] = sp - sn;
  bpr_tail_log_outside(sp - sn, a.B, a.lossrow[b], a.coef[b]);
  a.nodes[3 * b] = (int32_t)nu;
  a.nodes[3 * b + 1] = (int32_t)np;
  a.nodes[3 * b + 2] = (int32_t)nn;
}

// Gradient rows of E_final: occurrence o = 3b + t of node nodes[o] contributes c_b (i+ - i-) (t = 0, the user), c_b u (t = 1)
// or -c_b u (t = 2).  One wave per occurrence, pair_head.cuh's first-occurrence scheme; a later occurrence writes nothing.  The
// scheme is spelled out here: through the shared walk and register row the compiler fuses the three forms' multiply-adds
// differently per CH and the gradient moves by an ulp (profiles/pair_head/README.md).
template <int CH>
__global__ void __launch_bounds__(256) lgcn_pair_bwd_kernel(const f32x4* __restrict__ emb, int dv, const int32_t* __restrict__ nodes,
                                                            const float* __restrict__ coef, int n_occ, float gscale,
                                                            const float* __restrict__ gscale_dev, f32x4* __restrict__ grad) {
  const int lane = threadIdx.x & 63;
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (o >= n_occ) return;
  const int32_t node = nodes[o];
  for (int k0 = 0; k0 < o; k0 += 64) {
    const int k = k0 + lane;
    if (__ballot(k < o && nodes[k] == node)) return;
  }
  const float g = gscale * (gscale_dev ? gscale_dev[0] : 1.f);
  f32x4 s[CH];
#pragma unroll
  for (int h = 0; h < CH; ++h) s[h] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = o; k0 < n_occ; k0 += 64) {
    const int k = k0 + lane;
    unsigned long long m = __ballot(k < n_occ && nodes[k] == node);
    while (m) {
      const int oo = k0 + __builtin_ctzll(m);
      m &= m - 1;
      const int bb = oo / 3, t = oo - 3 * bb;
      const float c = coef[bb] * g;
      const int64_t n0 = nodes[3 * bb], n1 = nodes[3 * bb + 1], n2 = nodes[3 * bb + 2];
#pragma unroll
      for (int h = 0; h < CH; ++h) {
        const int ch = lane + h * 64;
        if (ch >= dv) continue;
        if (t == 0) s[h] += c * (emb[n1 * dv + ch] - emb[n2 * dv + ch]);
        else if (t == 1) s[h] += c * emb[n0 * dv + ch];
        else s[h] -= c * emb[n0 * dv + ch];
      }
    }
  }
#pragma unroll
  for (int h = 0; h < CH; ++h) {
    const int ch = lane + h * 64;
    if (ch < dv) grad[(int64_t)node * dv + ch] = s[h];
  }
}

static int lgcn_lanes_log2(int dv) {
  int lg = 0;
  while ((1 << lg) < dv && lg < 6) ++lg;
  return lg;
}

}  // namespace pxr

using namespace pxr;

extern "C" int64_t pxr_lgcn_spmm_ws_bytes(int64_t n_parts, int D) {
  if (n_parts < 0 || D <= 0 || D % 4) return -1;
  return n_parts * (int64_t)D * 4;
}

extern "C" int pxr_lgcn_spmm_f32(const int64_t* row_ptr, const int32_t* col, const float* w, int64_t n_rows, int D,
                                 const int32_t* split_row, const int32_t* split_part0, int n_split, const int32_t* part_owner,
                                 int n_parts, int part_len, const float* x, float* y, const float* acc_in, float* acc_out,
                                 float scale, void* ws, int64_t ws_bytes, void* stream) {
  PXR_REQUIRE(row_ptr && col && w && x, "pxr_lgcn_spmm_f32: null pointer");
  PXR_REQUIRE(y || acc_out, "pxr_lgcn_spmm_f32: neither y nor acc_out given");
  PXR_REQUIRE(n_rows > 0 && n_rows < (1ll << 31), "pxr_lgcn_spmm_f32: need 0 < n_rows < 2^31 (n_rows=%lld)", (long long)n_rows);
  PXR_REQUIRE(D > 0 && D % 4 == 0 && D <= 2048, "pxr_lgcn_spmm_f32: need D %% 4 == 0 and 0 < D <= 2048 (D=%d)", D);
  PXR_REQUIRE(part_len > 0 && n_split >= 0 && n_parts >= n_split, "pxr_lgcn_spmm_f32: bad split plan");
  PXR_REQUIRE(n_split == 0 || (split_row && split_part0 && part_owner), "pxr_lgcn_spmm_f32: split plan pointers missing");
  PXR_REQUIRE((const void*)x != (const void*)y && (const void*)x != (const void*)acc_out,
              "pxr_lgcn_spmm_f32: x must not alias y or acc_out (other rows still read it)");
  PXR_REQUIRE(n_parts == 0 || (ws && ws_bytes >= pxr_lgcn_spmm_ws_bytes(n_parts, D)), "pxr_lgcn_spmm_f32: workspace too small");
  const int64_t waves = n_rows + n_parts, blocks = (waves + 3) / 4;
  PXR_REQUIRE(blocks < (1ll << 31), "pxr_lgcn_spmm_f32: too many rows");
  SpmmArgs a{};
  a.row_ptr = row_ptr; a.col = col; a.w = w; a.n_rows = n_rows; a.dv = D / 4;
  a.split_row = split_row; a.split_part0 = split_part0; a.part_owner = part_owner;
  a.n_split = n_split; a.n_parts = n_parts; a.part_len = part_len;
  a.x = (const f32x4*)x; a.y = (f32x4*)y; a.acc_in = (const f32x4*)acc_in; a.acc_out = (f32x4*)acc_out; a.scale = scale;
  a.ws = (f32x4*)ws; a.status = pxr_status_word();
  a.lg = lgcn_lanes_log2(a.dv);                                    // dv > 64: all 64 lanes, CH chunks each
  hipStream_t st = (hipStream_t)stream;
  dispatch_ch<8>(a.dv, [&](auto ch) {
    hipLaunchKernelGGL(lgcn_spmm_kernel<decltype(ch)::value>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  });
  if (n_split > 0)
    hipLaunchKernelGGL(lgcn_spmm_combine_kernel, dim3((unsigned)((n_split + 3) / 4)), dim3(256), 0, st, a);
  return pxr_check_launch("pxr_lgcn_spmm_f32");
}

extern "C" int pxr_lgcn_pair_fwd_f32(const float* emb, int64_t n_users, int64_t n_items, int D, const int64_t* user,
                                     const int64_t* item, int B, float* diff, float* coef, float* lossrow, int32_t* nodes,
                                     float* loss, void* stream) {
  PXR_REQUIRE(emb && user && item && diff && coef && lossrow && nodes && loss, "pxr_lgcn_pair_fwd_f32: null pointer");
  PXR_REQUIRE(n_users > 0 && n_items > 0 && n_users + n_items < (1ll << 31), "pxr_lgcn_pair_fwd_f32: bad table size");
  PXR_REQUIRE(D > 0 && D % 4 == 0, "pxr_lgcn_pair_fwd_f32: need D %% 4 == 0 (D=%d)", D);
  PXR_REQUIRE(B > 0 && B <= (1 << 28), "pxr_lgcn_pair_fwd_f32: bad batch size %d", B);
  PairArgs a{};
  a.emb = (const f32x4*)emb; a.n_users = n_users; a.n_items = n_items; a.dv = D / 4; a.B = B;
  a.user = user; a.item = item; a.diff = diff; a.coef = coef; a.lossrow = lossrow; a.nodes = nodes;
  a.status = pxr_status_word();
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lgcn_pair_fwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, a);
  const int rc = pxr_check_launch("pxr_lgcn_pair_fwd_f32");
  if (rc) return rc;
  return pxr_bpr_loss_reduce(lossrow, B, 1, loss, stream);        // loss = (1/B) sum_b lossrow[b], fixed order
}

extern "C" int pxr_lgcn_pair_bwd_f32(const float* emb, int64_t n_nodes, int D, const int32_t* nodes, const float* coef, int B,
                                     float grad_scale, const float* grad_scale_dev, float* grad, void* stream) {
  PXR_REQUIRE(emb && nodes && coef && grad, "pxr_lgcn_pair_bwd_f32: null pointer");
  PXR_REQUIRE(n_nodes > 0 && n_nodes < (1ll << 31), "pxr_lgcn_pair_bwd_f32: bad table size");
  PXR_REQUIRE(D > 0 && D % 4 == 0 && D <= 2048, "pxr_lgcn_pair_bwd_f32: need D %% 4 == 0 and 0 < D <= 2048 (D=%d)", D);
  PXR_REQUIRE(B > 0 && B <= (1 << 28), "pxr_lgcn_pair_bwd_f32: bad batch size %d", B);
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(grad, 0, (size_t)n_nodes * D * 4, st) != hipSuccess) {
    pxr_set_error("pxr_lgcn_pair_bwd_f32: memset failed");
    return PXR_ERR_LAUNCH;
  }
  const int dv = D / 4, n_occ = 3 * B;
  dispatch_ch<8>(dv, [&](auto ch) {
    hipLaunchKernelGGL(lgcn_pair_bwd_kernel<decltype(ch)::value>, dim3((unsigned)((n_occ + 3) / 4)), dim3(256), 0, st,
                       (const f32x4*)emb, dv, nodes, coef, n_occ, grad_scale, grad_scale_dev, (f32x4*)grad);
  });
  return pxr_check_launch("pxr_lgcn_pair_bwd_f32");
}
