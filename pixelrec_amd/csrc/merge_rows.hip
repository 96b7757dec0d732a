// merge_rows.hip -- the data-parallel rank merge of the sparse table gradient.
//
// Data-parallel merge of W rank-local sparse gradients that are each ALREADY sorted and unique (the output of the
// segment sums of embed_grad.hip), concatenated as idx_all [W, cap] / rows_all [W, cap, D]; every list is ascending over its
// whole `cap` (unused tail slots hold ids >= n_table).  No second sort: a lower-bound search finds where an id sits in
// the other W-1 lists, the lowest rank holding an id owns its output slot and adds the other ranks' rows in rank
// order -- a fixed order that is the same on every replica, so replicas stay bit-identical.  The output is NOT
// compacted: slot e = (rank, i) carries (id, summed row) if that rank owns the id, else id 0 (= padding_idx, which
// every consumer skips); *n_out = W * cap.
#include "pxr_common.h"

namespace pxr {

// Where the W lists live.  Two layouts share the kernels: separate contiguous arrays idx_all [W, cap] / rows_all
// [W, cap, D] whose tails are PAD-terminated (counts == nullptr), and W packed blocks {ids[cap], int32 count, pad to
// 16 bytes, rows[cap][D]} as one all-gather delivers them (counts != nullptr: entries at or beyond a list's count are
// ignored, whatever they hold).
struct MergeSrc {
  const char* ids;    int64_t ids_stride;      // byte stride between consecutive ranks' lists
  const char* rows;   int64_t rows_stride;
  const char* counts; int64_t counts_stride;   // int32 per rank, or nullptr
  int32_t* status;                             // device status word: bit 1 is set when a list's count exceeds `cap`
};
__device__ __forceinline__ const int64_t* merge_ids(const MergeSrc& s, int q) {
  return reinterpret_cast<const int64_t*>(s.ids + (int64_t)q * s.ids_stride);
}
__device__ __forceinline__ const float* merge_rows(const MergeSrc& s, int q) {
  return reinterpret_cast<const float*>(s.rows + (int64_t)q * s.rows_stride);
}
__device__ __forceinline__ int merge_count(const MergeSrc& s, int q, int cap) {
  if (!s.counts) return cap;
  const int n = *reinterpret_cast<const int*>(s.counts + (int64_t)q * s.counts_stride);
  if (n > cap && s.status) atomicOr(s.status, PXR_STATUS_ROWS_OVERFLOW);   // rows beyond the exchanged capacity were cut off
  return n < 0 ? 0 : (n > cap ? cap : n);
}

__global__ void __launch_bounds__(256) merge_locate_kernel(MergeSrc s, int W, int cap, int64_t n_table,
                                                           int* __restrict__ pos) {
  const int64_t total = (int64_t)W * cap * W;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int64_t e = t / W;
    const int q = (int)(t - e * W);
    const int r = (int)(e / cap);
    const int i = (int)(e - (int64_t)r * cap);
    const int64_t key = i < merge_count(s, r, cap) ? merge_ids(s, r)[i] : 0;
    int p = -1;
    if (key > 0 && key < n_table) {
      if (q == r) {
        p = i;
      } else {
        const int64_t* list = merge_ids(s, q);
        const int nq = merge_count(s, q, cap);
        int lo = 0, hi = nq;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (list[mid] < key) lo = mid + 1; else hi = mid;
        }
        if (lo < nq && list[lo] == key) p = lo;
      }
    }
    pos[t] = p;
  }
}

// one wave per output slot
__global__ void __launch_bounds__(256) merge_sum_kernel(MergeSrc s, const int* __restrict__ pos, int W, int cap, int D,
                                                        float scale, int64_t* __restrict__ out_idx,
                                                        float* __restrict__ out_rows, int32_t* __restrict__ n_out) {
  const int lane = threadIdx.x & 63;
  const int64_t E = (int64_t)W * cap;
  if (blockIdx.x == 0 && threadIdx.x == 0) *n_out = (int32_t)E;
  const int dv = D >> 2;
  for (int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); e < E; e += (int64_t)gridDim.x * 4) {
    const int r = (int)(e / cap);
    const int p = lane < W ? pos[e * W + lane] : -1;
    const unsigned long long have = __ballot(p >= 0);
    const bool owner = have != 0ull && (__ffsll((long long)have) - 1) == r;   // wave-uniform
    if (!owner) {
      if (lane == 0) out_idx[e] = 0;
      continue;
    }
    for (int c = lane; c < dv; c += 64) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      unsigned long long m = have;
      while (m) {
        const int q = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int pq = __shfl(p, q, 64);
        const float4 v = *reinterpret_cast<const float4*>(merge_rows(s, q) + (int64_t)pq * D + c * 4);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
      acc.x *= scale; acc.y *= scale; acc.z *= scale; acc.w *= scale;
      *reinterpret_cast<float4*>(out_rows + e * D + c * 4) = acc;
    }
    if (lane == 0) out_idx[e] = merge_ids(s, r)[e - (int64_t)r * cap];
  }
}

}  // namespace pxr

using namespace pxr;

extern "C" int64_t pxr_merge_rows_ws_bytes(int W, int64_t cap) {
  return ((int64_t)W * cap * W * 4 + 255) & ~(int64_t)255;
}

// The shape and workspace checks of entry point `what` (cap: the row capacity of the lists as exchanged), then the two launches.
static int launch_merge(const char* what, const MergeSrc& src, int W, int64_t cap, int D, int64_t n_table, float scale,
                        int64_t* out_idx, float* out_rows, int32_t* n_out_dev, void* ws, int64_t ws_bytes, hipStream_t st) {
  PXR_REQUIRE(W >= 1 && W <= 64 && cap > 0 && (int64_t)W * cap * W < (1ll << 31) && D > 0 && D % 4 == 0 && n_table > 0,
              "%s: bad shape", what);
  if (pxr_merge_rows_ws_bytes(W, cap) > ws_bytes) { pxr_set_error("%s: workspace too small", what); return PXR_ERR_WORKSPACE; }
  const int64_t total = (int64_t)W * cap * W, E = (int64_t)W * cap;
  int64_t b1 = (total + 255) / 256; if (b1 > 8192) b1 = 8192;
  hipLaunchKernelGGL(merge_locate_kernel, dim3((unsigned)b1), dim3(256), 0, st, src, W, (int)cap, n_table, (int*)ws);
  int64_t b2 = (E + 3) / 4; if (b2 > 8192) b2 = 8192;
  hipLaunchKernelGGL(merge_sum_kernel, dim3((unsigned)b2), dim3(256), 0, st, src, (const int*)ws, W, (int)cap, D, scale,
                     out_idx, out_rows, n_out_dev);
  return pxr_check_launch(what);
}

// See merge_locate_kernel: merges W sorted-unique sparse gradients without re-sorting.
extern "C" int pxr_merge_sorted_rows_f32(const int64_t* idx_all, const float* rows_all, int W, int64_t cap, int D,
                                         int64_t n_table, float scale, int64_t* out_idx, float* out_rows,
                                         int32_t* n_out_dev, void* ws, int64_t ws_bytes, void* stream) {
  PXR_REQUIRE(idx_all && rows_all && out_idx && out_rows && n_out_dev && ws, "pxr_merge_sorted_rows_f32: null pointer");
  MergeSrc src{};
  src.ids = (const char*)idx_all;   src.ids_stride = cap * 8;
  src.rows = (const char*)rows_all; src.rows_stride = cap * (int64_t)D * 4;
  return launch_merge("pxr_merge_sorted_rows_f32", src, W, cap, D, n_table, scale, out_idx, out_rows, n_out_dev, ws, ws_bytes,
                      (hipStream_t)stream);
}

// The packed block one rank contributes to a ONE-collective exchange: {int64 ids[cap]; int32 count; zero padding up to a
// 16-byte boundary; float rows[cap][D]}.
extern "C" int64_t pxr_packed_rows_offset(int64_t cap) { return ((cap + 1) * 8 + 15) & ~(int64_t)15; }
extern "C" int64_t pxr_packed_rows_bytes(int64_t cap, int D) { return pxr_packed_rows_offset(cap) + cap * (int64_t)D * 4; }

extern "C" int pxr_merge_packed_rows_f32(const void* packed_all, int W, int64_t cap, int D, int64_t n_table, float scale,
                                         int64_t* out_idx, float* out_rows, int32_t* n_out_dev, void* ws,
                                         int64_t ws_bytes, void* stream) {
  PXR_REQUIRE(packed_all && out_idx && out_rows && n_out_dev && ws, "pxr_merge_packed_rows_f32: null pointer");
  PXR_REQUIRE(((uintptr_t)packed_all & 15) == 0, "pxr_merge_packed_rows_f32: packed_all must be 16-byte aligned");
  const int64_t block = pxr_packed_rows_bytes(cap, D);
  MergeSrc src{};
  src.ids = (const char*)packed_all;                                   src.ids_stride = block;
  src.rows = (const char*)packed_all + pxr_packed_rows_offset(cap);    src.rows_stride = block;
  src.counts = (const char*)packed_all + cap * 8;                      src.counts_stride = block;
  return launch_merge("pxr_merge_packed_rows_f32", src, W, cap, D, n_table, scale, out_idx, out_rows, n_out_dev, ws, ws_bytes,
                      (hipStream_t)stream);
}

// The TWO-collective exchange with a reduced row capacity: every rank all-gathers the HEAD of its packed block ({ids[cap],
// count, pad} = pxr_packed_rows_offset(cap) bytes) and only the first `cap_x` rows.  cap_x is a bound on the unique rows
// of a batch that the caller knows (e.g. from the batcher); a count above it sets bit 1 of the status word
// (pxr_set_status_word) -- the host raises -- and the list is cut at cap_x.  Output: W * cap_x slots.
extern "C" int pxr_merge_split_rows_f32(const void* heads_all, const float* rows_all, int W, int64_t cap, int64_t cap_x,
                                        int D, int64_t n_table, float scale, int64_t* out_idx, float* out_rows,
                                        int32_t* n_out_dev, void* ws, int64_t ws_bytes, void* stream) {
  PXR_REQUIRE(heads_all && rows_all && out_idx && out_rows && n_out_dev && ws, "pxr_merge_split_rows_f32: null pointer");
  PXR_REQUIRE(cap > 0 && cap_x <= cap, "pxr_merge_split_rows_f32: bad shape");   // the rest of the shape: launch_merge, on cap_x
  PXR_REQUIRE((((uintptr_t)heads_all | (uintptr_t)rows_all) & 15) == 0, "pxr_merge_split_rows_f32: unaligned input");
  const int64_t head = pxr_packed_rows_offset(cap);
  MergeSrc src{};
  src.ids = (const char*)heads_all;               src.ids_stride = head;
  src.counts = (const char*)heads_all + cap * 8;  src.counts_stride = head;
  src.rows = (const char*)rows_all;               src.rows_stride = cap_x * (int64_t)D * 4;
  src.status = pxr_status_word();
  return launch_merge("pxr_merge_split_rows_f32", src, W, cap_x, D, n_table, scale, out_idx, out_rows, n_out_dev, ws, ws_bytes,
                      (hipStream_t)stream);
}
