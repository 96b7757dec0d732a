// visrank.hip -- VISRANK (model/ViNet/visrank.py): training-free visual ranking, fused cosine scoring + history reduction + top-K.
//
// Reference, per user (visrank.py:37-56, one user per call):
//   w = history[-50:];  S[r, j] = cosine_similarity(v_feat[w[r]], v_feat[j])          [h, N]  (a [h, N, F] product in torch)
//   score[j] = mean of the k largest of S[:, j]   (k = min(top_num, h) | 1 | h);  score[0] = -inf
//   trainer: scores[(history_u, history_i)] = -inf over the FULL history, torch.topk(scores, max(topk))
// Here: the rows are normalised once per model (visrank_unit_rows_kernel), so S is a plain product of unit rows.  Every workgroup
// owns TWO users -- their window rows gathered into a 128-row panel, 64 rows per user, left-padded with zero rows -- times one
// contiguous range of item tiles, runs the fp32-operand MFMA main loop of gemm_f32.cuh per 128 x 128 tile (the A operand gathered
// through a row list, gemm_mainloop's A_GATHER), drops the tile into LDS and gives each of the 256 threads one (user, column) pair:
// the thread scans the column's h valid rows, keeps the k largest in a register list (TK entries, fully unrolled), takes their mean,
// applies the masks (column 0, the ragged edge, the user's full history as a bitmap in LDS) and inserts into its private top-K list.
// The 64 lists of a wave are merged with wave shuffles into one list per (user, split, wave); the shared merge kernel
// (topk_select.cuh: pxr_topk_merge) merges those.
// S never reaches HBM; the workspace holds the row list, the window lengths and the partial lists.
//
// Bad input (a window or history id outside [0, N), a 0 inside the window's valid tail, an empty window) is found by the first
// kernel, which sets PXR_STATUS_BAD_INDEX and a flag in the workspace: the later kernels return at once, the outputs are untouched.
#include "gemm_f32.cuh"
#include "topk_select.cuh"

namespace pxr {

constexpr int VR_BM = 128, VR_BN = 128;
constexpr int VR_ROWS = 64;                    // panel rows per user (H <= 64)
constexpr int VR_UPT = VR_BM / VR_ROWS;        // users per tile
constexpr int VR_LD = VR_BN + 1;               // score-tile row stride in LDS (odd: the accumulator scatter is conflict-free)
using VrCfg = GemmCfg<VR_BM, VR_BN, true, true>;
constexpr int VR_SMEM_FLOATS = (2 * VrCfg::STAGE > VR_BM * VR_LD) ? 2 * VrCfg::STAGE : VR_BM * VR_LD;
constexpr int VR_BITMAP_WORDS = VR_UPT * (VR_BN / 32);

struct VisrankArgs {
  const float* unit;                      // [N, F] unit rows
  const int64_t* window;                  // [B, H] left-padded with 0
  const int* hist_ptr;                    // [B+1] CSR offsets (may be null)
  const int64_t* hist_items;
  int* bad;                               // workspace: != 0 once bad input was met
  int* hlen;                              // workspace [B]: valid window rows per user
  int* rows;                              // workspace [row_blocks * 128]: table row of every panel row, -1 = a row of zeros
  float* part_val; int* part_idx;         // workspace [B, n_split * 2, KT]
  int32_t* status;
  int B, H, N, F, top_k, tiles_n, n_split, row_blocks;
};

// unit[i] = feat[i] / max(||feat[i]||_2, eps): one wave per row
__global__ void __launch_bounds__(256) visrank_unit_rows_kernel(const float* __restrict__ feat, int64_t N, int F, float eps,
                                                                float* __restrict__ unit) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* x = feat + row * F;
  float ss = 0.f;
  for (int k = lane * 4; k < F; k += 256) {
    const float4 v = *reinterpret_cast<const float4*>(x + k);
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  const float nrm = fmaxf(sqrtf(wave_sum(ss)), eps);
  float* y = unit + row * F;
  for (int k = lane * 4; k < F; k += 256) {
    const float4 v = *reinterpret_cast<const float4*>(x + k);
    *reinterpret_cast<float4*>(y + k) = make_float4(v.x / nrm, v.y / nrm, v.z / nrm, v.w / nrm);
  }
}

// one wave per panel slot of 64 rows (users past B: all -1): row list, window length, input checks
__global__ void __launch_bounds__(64) visrank_prep_kernel(VisrankArgs a) {
  const int u = blockIdx.x, r = threadIdx.x;
  if (u >= a.B) { a.rows[u * VR_ROWS + r] = -1; return; }
  const int slot = a.H - VR_ROWS + r;
  const int64_t id = slot >= 0 ? a.window[(int64_t)u * a.H + slot] : 0;
  const bool valid = id != 0;
  bool bad = id < 0 || id >= a.N;
  // left padding: the valid rows are the LAST h of the panel, h >= 1
  const unsigned long long m = __ballot(valid);
  const int h = __popcll(m);
  const unsigned long long want = h == 0 ? 0ull : (h == 64 ? ~0ull : (~0ull << (64 - h)));
  bad |= (m != want) || h == 0;
  bad |= hist_ids_bad<64>(a.hist_ptr, a.hist_items, u, a.N, r);
  a.rows[u * VR_ROWS + r] = (valid && !bad) ? (int)id : -1;
  if (r == 0) a.hlen[u] = h;
  if (__any(bad) && r == 0) raise_bad_input(a.bad, a.status);
}

// KT = length of the top-K lists; TK = length of the k-largest list of the history reduction (0: the mean over all h rows)
// (K <= 16: two workgroups per CU, so that one's column scan runs under the other's MFMAs; the 64 list registers of KT = 32 do not fit)
template <int KT, int TK>
__global__ void __launch_bounds__(GEMM_THREADS, (KT <= 16 ? 2 : 1)) visrank_topk_kernel(VisrankArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[VR_SMEM_FLOATS + VR_BITMAP_WORDS];
  if (*a.bad) return;
  unsigned* bitmap = reinterpret_cast<unsigned*>(smem + VR_SMEM_FLOATS);
  const int tid = threadIdx.x;
  const int t = xcd_remap(blockIdx.x, a.row_blocks * a.n_split);
  const int rb = t % a.row_blocks, sp = t / a.row_blocks;   // row-block fastest: neighbours share the item tiles
  const int m0 = rb * VR_BM, u0 = rb * VR_UPT;
  const TileRange tr = split_tile_range(a.tiles_n, a.n_split, sp);

  const int my_u = tid >> 7, my_c = tid & 127;              // (user in tile, column): the user is wave-uniform
  const int user = u0 + my_u;
  const int h = user < a.B ? a.hlen[user] : 0;
  const int k = TK == 0 ? h : min(a.top_k, h);
  TopList<KT> top;
  top.init();

  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, hh = lane >> 5, r = lane & 31;
  int hb = 0, hm = 0, he = 0;
  if (a.hist_ptr) {
    hb = a.hist_ptr[u0];
    hm = a.hist_ptr[min(a.B, u0 + 1)];
    he = a.hist_ptr[min(a.B, u0 + VR_UPT)];
  }

  for (int tn = tr.tn0; tn < tr.tn1; ++tn) {
    const int n0 = tn * VR_BN;
    if (tid < VR_BITMAP_WORDS) bitmap[tid] = 0u;
    typename VrCfg::Acc accs;
    gemm_mainloop<VR_BM, VR_BN, true, true, false, 1, 1, 2, 0, false, true>(accs, a.unit, (int64_t)a.F, a.unit, (int64_t)a.F,
                                                                            a.row_blocks * VR_BM, a.N, 0, a.F, m0, n0, smem,
                                                                            nullptr, a.rows);
    // (the main loop starts and ends with barriers: the zeroed bitmap is visible, the staging buffers are free) -> tile in LDS
#pragma unroll
    for (int j = 0; j < VrCfg::TN; ++j) {
      const int cl = wn * VrCfg::WN + j * 32 + r;
#pragma unroll
      for (int i = 0; i < VrCfg::TM; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int rl = wm * VrCfg::WM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
          smem[rl * VR_LD + cl] = accs.v[i][j][e];
        }
    }
    // history mask (trainer.py:335-336) over the users' FULL histories: pairs of this tile as bits
    hist_bitmap_rows<VR_BN, GEMM_THREADS>(bitmap, a.hist_items, hb, he, n0, tid, [hm](int p) { return p >= hm ? 1 : 0; });
    __syncthreads();
    const int col = n0 + my_c;
    if (user < a.B && item_alive(bitmap + my_u * (VR_BN / 32), col, my_c, a.N)) {
      const float* colp = smem + (my_u * VR_ROWS) * VR_LD + my_c;
      float s = 0.f;
      if constexpr (TK == 0) {
        for (int q = VR_ROWS - h; q < VR_ROWS; ++q) s += colp[q * VR_LD];
      } else {
        float v[TK];
#pragma unroll
        for (int i = 0; i < TK; ++i) v[i] = -INFINITY;
        for (int q = VR_ROWS - h; q < VR_ROWS; ++q) {
          const float x = colp[q * VR_LD];
          if (x > v[TK - 1]) {
            v[TK - 1] = x;
#pragma unroll
            for (int i = TK - 1; i > 0; --i)
              if (v[i] > v[i - 1]) { const float tv = v[i]; v[i] = v[i - 1]; v[i - 1] = tv; }
          }
        }
#pragma unroll
        for (int i = 0; i < TK; ++i)
          if (i < k) s += v[i];
      }
      top.insert(s / (float)k, col);
    }
    __syncthreads();
  }
  if (user >= a.B) return;                                  // wave-uniform
  // the wave's 64 lists -> one list per (user, split, wave)
  const int64_t o = ((int64_t)user * (a.n_split * 2) + (sp * 2 + (wave & 1))) * KT;
  wave_collapse_lists(top, lane, a.part_val + o, a.part_idx + o);
}

static int vr_row_blocks(int B) { return (B + VR_UPT - 1) / VR_UPT; }
static int vr_tiles(int N) { return (N + VR_BN - 1) / VR_BN; }
static int64_t vr_hlen_bytes(int B) { return a256((int64_t)B * 4); }
static int64_t vr_own_bytes(int B) { return vr_hlen_bytes(B) + a256((int64_t)vr_row_blocks(B) * VR_BM * 4); }
static bool vr_shape_ok(int B, int H, int N, int K) {
  return B > 0 && B <= (1 << 22) && H >= 1 && H <= VR_ROWS && N > 0 && K >= 1 && K <= 32;
}

}  // namespace pxr

using namespace pxr;

extern "C" int pxr_visrank_unit_rows_f32(const float* feat, int64_t N, int F, float eps, float* unit, void* stream) {
  PXR_REQUIRE(feat && unit, "pxr_visrank_unit_rows_f32: null pointer");
  PXR_REQUIRE(N > 0 && F > 0 && F % 4 == 0 && eps > 0.f, "pxr_visrank_unit_rows_f32: bad shape (F %% 4 == 0, eps > 0)");
  PXR_REQUIRE(((((uintptr_t)feat) | ((uintptr_t)unit)) & 15) == 0, "pxr_visrank_unit_rows_f32: operands must be 16-byte aligned");
  PXR_REQUIRE((N + 3) / 4 < (1ll << 31), "pxr_visrank_unit_rows_f32: too many rows");
  hipLaunchKernelGGL(visrank_unit_rows_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, feat, N, F, eps, unit);
  return pxr_check_launch("pxr_visrank_unit_rows_f32");
}

// input flag | window lengths | row list | partial values | partial ids
extern "C" int64_t pxr_visrank_topk_ws_bytes(int B, int H, int N, int K) {
  if (!vr_shape_ok(B, H, N, K)) return -1;
  const int64_t cand = (int64_t)topk_pick_split(vr_row_blocks(B), vr_tiles(N)) * 2 * pick_kt(K);
  return topk_ws_bytes(vr_own_bytes(B), B, cand);
}

extern "C" int pxr_visrank_topk_f32(const float* unit, int N, int F, const int64_t* window, int B, int H, int top_k,
                                    const int32_t* hist_ptr, const int64_t* hist_items, int K, int64_t* topk_idx, float* topk_val,
                                    void* ws, int64_t ws_bytes, void* stream) {
  PXR_REQUIRE(unit && window && topk_idx && topk_val && ws, "pxr_visrank_topk_f32: null pointer");
  PXR_REQUIRE(vr_shape_ok(B, H, N, K), "pxr_visrank_topk_f32: bad shape (1 <= H <= 64, 1 <= K <= 32)");
  PXR_REQUIRE(F > 0 && F % 4 == 0 && (int64_t)N * F * 4 < 0x7FFFFFF0ll, "pxr_visrank_topk_f32: F %% 4 == 0 and a feature matrix below 2 GiB");
  PXR_REQUIRE((((uintptr_t)unit) & 15) == 0, "pxr_visrank_topk_f32: unit must be 16-byte aligned");
  PXR_REQUIRE(top_k >= 0 && top_k <= 16, "pxr_visrank_topk_f32: top_k must be in [0, 16] (0 = the mean over the window)");
  PXR_REQUIRE(!hist_ptr || hist_items, "pxr_visrank_topk_f32: hist_ptr without hist_items");
  if (pxr_visrank_topk_ws_bytes(B, H, N, K) > ws_bytes) { pxr_set_error("pxr_visrank_topk_f32: workspace too small"); return PXR_ERR_WORKSPACE; }
  const int kt = pick_kt(K);
  VisrankArgs a{};
  a.unit = unit; a.window = window; a.hist_ptr = hist_ptr; a.hist_items = hist_items;
  a.B = B; a.H = H; a.N = N; a.F = F; a.top_k = top_k;
  a.row_blocks = vr_row_blocks(B);
  a.tiles_n = vr_tiles(N);
  a.n_split = topk_pick_split(a.row_blocks, a.tiles_n);
  a.status = pxr_status_word();
  const int64_t cand = (int64_t)a.n_split * 2 * kt;
  const TopkWs w = topk_ws_carve(ws, vr_own_bytes(B), B, cand);
  a.bad = w.bad; a.part_val = w.part_val; a.part_idx = w.part_idx;
  a.hlen = (int*)w.own;
  a.rows = (int*)(w.own + vr_hlen_bytes(B));
  hipStream_t st = (hipStream_t)stream;
  if (int rc = topk_ws_clear_flag(w, "pxr_visrank_topk_f32(memset)", st)) return rc;
  hipLaunchKernelGGL(visrank_prep_kernel, dim3(a.row_blocks * VR_UPT), dim3(64), 0, st, a);
  if (int rc = pxr_check_launch("pxr_visrank_topk_f32(prep)")) return rc;
  const dim3 grid(a.row_blocks * a.n_split);
  const int tk = top_k == 0 ? 0 : (top_k == 1 ? 1 : (top_k <= 4 ? 4 : 16));
  topk_for_kt(kt, [&](auto k) {
    constexpr int KT = decltype(k)::value;
    switch (tk) {
      case 0: hipLaunchKernelGGL((visrank_topk_kernel<KT, 0>), grid, dim3(GEMM_THREADS), 0, st, a); break;
      case 1: hipLaunchKernelGGL((visrank_topk_kernel<KT, 1>), grid, dim3(GEMM_THREADS), 0, st, a); break;
      case 4: hipLaunchKernelGGL((visrank_topk_kernel<KT, 4>), grid, dim3(GEMM_THREADS), 0, st, a); break;
      default: hipLaunchKernelGGL((visrank_topk_kernel<KT, 16>), grid, dim3(GEMM_THREADS), 0, st, a); break;
    }
  });
  return topk_ws_merge(w, B, cand, K, topk_idx, topk_val, "pxr_visrank_topk_f32", "pxr_visrank_topk_f32(merge)", stream);
}
