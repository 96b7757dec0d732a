// topk_select.cuh -- the selection core shared by the fused "score the catalogue, keep the K best" kernels
// (score_topk.hip, visrank.hip, din.hip, widedeep.hip): the sorted register list, the collapse of a wave's 64 lists into one, the
// owner search and bitmap of the history mask, and the frame of a walk over item tiles -- the tile range of a split, the alive
// test, the input flag of the prep kernels, and on the host the split rule, the list-length dispatch and the workspace of flag
// and candidate buffers.  No kernel lives here: the one merge kernel (topk_merge_kernel) is score_topk.hip's, reached from the
// other translation units through pxr_topk_merge.  No helper holds a barrier: where a kernel synchronises is part of its schedule.
//
// Invariant of every list and of everything merged from lists: a slot's value is -inf exactly when its id is -1.  init() and
// pop() write the pair (-inf, -1); insert() admits x only if x > v[KT-1] >= -inf, so neither -inf nor NaN ever enters with an id.
#pragma once
#include <type_traits>

#include "pxr_common.h"

// One wave per user: out[u, 0:K] = the K best of part[u, 0:n_cand], descending by value, ties by ascending position
// (topk_merge_kernel, score_topk.hip).  skip (device, may be null): the kernel returns at once when *skip != 0, the outputs
// untouched.  Returns pxr_check_launch(what).  Internal, not in the ABI.
int pxr_topk_merge(const int* skip, const float* part_val, const int* part_idx, int B, int n_cand, int K, int64_t* out_idx,
                   float* out_val, const char* what, void* stream);

namespace pxr {

// length of the register lists that serve a top-K request (0: K is out of range)
static inline int pick_kt(int K) { return K <= 10 ? 10 : (K <= 16 ? 16 : (K <= 32 ? 32 : 0)); }
static inline int64_t a256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// f(std::integral_constant<int, KT>) for kt = pick_kt(K): the one place a list length becomes a template argument
template <class F>
static inline void topk_for_kt(int kt, F&& f) {
  switch (kt) {
    case 10: f(std::integral_constant<int, 10>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    default: f(std::integral_constant<int, 32>{}); break;
  }
}

// into how many ranges the item tiles are split; units = the workgroups that one range takes (users or row blocks).
// About two rounds of the chip: one or two resident workgroups per CU.
static inline int topk_pick_split(int units, int tiles_n) {
  int s = (512 + units - 1) / units;
  if (s > tiles_n) s = tiles_n;
  return s < 1 ? 1 : s;
}

// ---- the workspace of a fused top-k with an input check: 256 B flag (!= 0 once bad input was met) | the model's own buffers
// (own_bytes, a sum of a256 terms) | candidate values | candidate ids, [B, cand] each
static inline int64_t topk_ws_bytes(int64_t own_bytes, int B, int64_t cand) { return 256 + own_bytes + 2 * a256((int64_t)B * cand * 4); }
struct TopkWs {
  int* bad;
  char* own;
  float* part_val;
  int* part_idx;
};
static inline TopkWs topk_ws_carve(void* ws, int64_t own_bytes, int B, int64_t cand) {
  char* w = (char*)ws;
  return TopkWs{(int*)w, w + 256, (float*)(w + 256 + own_bytes), (int*)(w + 256 + own_bytes + a256((int64_t)B * cand * 4))};
}

#ifdef __HIPCC__
// the flag is cleared ahead of the prep kernel; who = the entry point, for the error text
static inline int topk_ws_clear_flag(const TopkWs& w, const char* who, hipStream_t st) {
  if (hipMemsetAsync(w.bad, 0, 256, st) != hipSuccess) return pxr_check_launch(who);
  return PXR_OK;
}
// behind the scoring kernel's launch: its launch check, then the merge of the [B, cand] candidates (skipped on bad input)
static inline int topk_ws_merge(const TopkWs& w, int B, int64_t cand, int K, int64_t* topk_idx, float* topk_val, const char* who,
                                const char* who_merge, void* stream) {
  if (int rc = pxr_check_launch(who)) return rc;
  return pxr_topk_merge(w.bad, w.part_val, w.part_idx, B, (int)cand, K, topk_idx, topk_val, who_merge, stream);
}

template <int KT>
struct TopList {
  float v[KT];
  int i[KT];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int k = 0; k < KT; ++k) { v[k] = -INFINITY; i[k] = -1; }
  }
  // sorted descending; v[KT-1] is the admission threshold
  __device__ __forceinline__ void insert(float x, int id) {
    if (!(x > v[KT - 1])) return;
    v[KT - 1] = x; i[KT - 1] = id;
#pragma unroll
    for (int k = KT - 1; k > 0; --k) {
      if (v[k] > v[k - 1]) {
        const float tv = v[k]; v[k] = v[k - 1]; v[k - 1] = tv;
        const int ti = i[k]; i[k] = i[k - 1]; i[k - 1] = ti;
      }
    }
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int k = 0; k + 1 < KT; ++k) { v[k] = v[k + 1]; i[k] = i[k + 1]; }
    v[KT - 1] = -INFINITY; i[KT - 1] = -1;
  }
};

// the wave's 64 lists -> one, written to out_val / out_idx [KT]: KT rounds of (best head of the wave: the larger value, among
// equal values the lower lane), the winner pops.  All 64 lanes must be active; the lists are consumed.
template <int KT>
__device__ __forceinline__ void wave_collapse_lists(TopList<KT>& top, int lane, float* out_val, int* out_idx) {
  for (int kk = 0; kk < KT; ++kk) {
    float bv = top.v[0];
    int bl = lane;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off, 64);
      const int ol = __shfl_xor(bl, off, 64);
      if (ov > bv || (ov == bv && ol < bl)) { bv = ov; bl = ol; }
    }
    if (lane == bl) {
      out_val[kk] = top.v[0];
      out_idx[kk] = top.i[0];
      top.pop();
    }
  }
}

// owner of history pair p: the user u in [u_first, u_last] with hist_ptr[u] <= p < hist_ptr[u+1]
__device__ __forceinline__ int hist_owner(const int* hist_ptr, int p, int u_first, int u_last) {
  int lo = u_first, hi = u_last;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (hist_ptr[mid] <= p) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- the walk of one workgroup over the item tiles of split sp: tiles [tn0, tn1), ceil(tiles_n / n_split) per split -- the last
// splits own fewer or none
struct TileRange {
  int tn0, tn1;
};
__device__ __forceinline__ TileRange split_tile_range(int tiles_n, int n_split, int sp) {
  const int per = (tiles_n + n_split - 1) / n_split;
  return TileRange{sp * per, min(tiles_n, sp * per + per)};
}

// whether item (= tile start + il) may enter a list: inside the catalogue, not the padding item 0, its bit of the user's bitmap
// row clear
__device__ __forceinline__ bool item_alive(const unsigned* bitmap_row, int item, int il, int N) {
  return item < N && item != 0 && !((bitmap_row[il >> 5] >> (il & 31)) & 1u);
}

// prep kernels: whether one of this thread's share (NT threads) of user u's history ids lies outside [0, N) ...
template <int NT>
__device__ __forceinline__ bool hist_ids_bad(const int* hist_ptr, const int64_t* hist_items, int u, int N, int tid) {
  bool bad = false;
  if (hist_ptr) {
    const int hb = hist_ptr[u], he = hist_ptr[u + 1];
    for (int p = hb + tid; p < he; p += NT) {
      const int64_t it = hist_items[p];
      bad |= it < 0 || it >= N;
    }
  }
  return bad;
}
// ... and the raise: the workspace flag stops the later kernels of the call, the status word reaches ops.raise_on_bad_indices
__device__ __forceinline__ void raise_bad_input(int* bad, int32_t* status) {
  *bad = 1;
  if (status) atomicOr(status, PXR_STATUS_BAD_INDEX);
}

// ---- the history mask of a workgroup that owns USERS users x a range of TILE_M-item tiles, as a bitmap in LDS:
// bitmap[user_local * (TILE_M / 32) + word], zeroed by the kernel before each fill.  hb / he = the pairs of the workgroup's
// users (hist_ptr[u0], hist_ptr[min(B, u0 + USERS)]), NT = threads of the workgroup.  The helpers hold no barrier: where the
// kernel synchronises is part of its schedule.
constexpr int ST4_HIST_CAP = 2048;   // history pairs of the workgroup's (users x its item range) kept in LDS

// per tile, from the global pairs hb..he: every pair whose item lies in [i0, i0 + TILE_M), into bitmap row row_of(p) -- a
// workgroup with one user passes 0, one with two users a comparison with the second user's first pair
template <int TILE_M, int NT, class RowOf>
__device__ __forceinline__ void hist_bitmap_rows(unsigned* bitmap, const int64_t* hist_items, int hb, int he, int i0, int tid,
                                                 RowOf row_of) {
  for (int p = hb + tid; p < he; p += NT) {
    const int64_t it = hist_items[p];
    if (it >= i0 && it < i0 + TILE_M) {
      const int il = (int)(it - i0);
      atomicOr(&bitmap[row_of(p) * (TILE_M / 32) + (il >> 5)], 1u << (il & 31));
    }
  }
}
// ... with the owner search for the row
template <int TILE_M, int USERS, int NT>
__device__ __forceinline__ void hist_bitmap_from_pairs(unsigned* bitmap, const int* hist_ptr, const int64_t* hist_items, int hb, int he,
                                                       int u0, int B, int i0, int tid) {
  hist_bitmap_rows<TILE_M, NT>(bitmap, hist_items, hb, he, i0, tid,
                               [=](int p) { return hist_owner(hist_ptr, p, u0, min(B, u0 + USERS) - 1) - u0; });
}

// once per workgroup: the pairs whose item lies in the workgroup's range [r_lo, r_hi), owner resolved, packed as
// (user_local << 20) | (item - r_lo) into hlist[ST4_HIST_CAP]; *hcount (zeroed by the kernel, a barrier before and after this
// call) counts every such pair, also those past the capacity
template <int USERS, int NT>
__device__ __forceinline__ void hist_list_collect(unsigned* hlist, int* hcount, const int* hist_ptr, const int64_t* hist_items, int hb,
                                                  int he, int u0, int B, int64_t r_lo, int64_t r_hi, int tid) {
  for (int p = hb + tid; p < he; p += NT) {
    const int64_t it = hist_items[p];
    if (it >= r_lo && it < r_hi) {
      const int lo = hist_owner(hist_ptr, p, u0, min(B, u0 + USERS) - 1);
      const int pos = atomicAdd(hcount, 1);
      if (pos < ST4_HIST_CAP) hlist[pos] = ((unsigned)(lo - u0) << 20) | (unsigned)(it - r_lo);
    }
  }
}
// whether the list holds every pair of the range: none dropped, and the packed pair's 20 bits cover the item offset inside the
// range (a wider range -- few splits over a huge catalogue -- would run into the user field).  Else: the global pairs per tile.
__device__ __forceinline__ bool hist_list_ok(int n_hist, int64_t r_lo, int64_t r_hi) {
  return n_hist <= ST4_HIST_CAP && (r_hi - r_lo) <= (1ll << 20);
}

// per tile: from the list when list_ok, otherwise from the global pairs
template <int TILE_M, int USERS, int NT>
__device__ __forceinline__ void hist_bitmap_fill(unsigned* bitmap, bool list_ok, const unsigned* hlist, int n_hist, int64_t r_lo,
                                                 const int* hist_ptr, const int64_t* hist_items, int hb, int he, int u0, int B, int i0,
                                                 int tid) {
  if (list_ok) {
    const unsigned off0 = (unsigned)(i0 - (int)r_lo);
    for (int q = tid; q < n_hist; q += NT) {
      const unsigned e = hlist[q], off = e & 0xFFFFFu;
      if (off >= off0 && off < off0 + TILE_M) {
        const int il = (int)(off - off0);
        atomicOr(&bitmap[(e >> 20) * (TILE_M / 32) + (il >> 5)], 1u << (il & 31));
      }
    }
  } else {
    hist_bitmap_from_pairs<TILE_M, USERS, NT>(bitmap, hist_ptr, hist_items, hb, he, u0, B, i0, tid);
  }
}
#endif  // __HIPCC__

}  // namespace pxr
