// topk_select.cuh -- the selection core shared by the fused "score the catalogue, keep the K best" kernels
// (score_topk.hip, visrank.hip, din.hip): the sorted register list, the collapse of a wave's 64 lists into one, the owner
// search and bitmap of the history mask, and the host helpers that size the lists.  No kernel lives here: the one merge
// kernel (topk_merge_kernel) is score_topk.hip's, reached from the other translation units through pxr_topk_merge.
//
// Invariant of every list and of everything merged from lists: a slot's value is -inf exactly when its id is -1.  init() and
// pop() write the pair (-inf, -1); insert() admits x only if x > v[KT-1] >= -inf, so neither -inf nor NaN ever enters with an id.
#pragma once
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

#ifdef __HIPCC__
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

// ---- the history mask of a workgroup that owns USERS users x a range of TILE_M-item tiles, as a bitmap in LDS:
// bitmap[user_local * (TILE_M / 32) + word], zeroed by the kernel before each fill.  hb / he = the pairs of the workgroup's
// users (hist_ptr[u0], hist_ptr[min(B, u0 + USERS)]), NT = threads of the workgroup.  The helpers hold no barrier: where the
// kernel synchronises is part of its schedule.
constexpr int ST4_HIST_CAP = 2048;   // history pairs of the workgroup's (users x its item range) kept in LDS

// per tile, from the global pairs: every pair of the workgroup's users whose item lies in [i0, i0 + TILE_M)
template <int TILE_M, int USERS, int NT>
__device__ __forceinline__ void hist_bitmap_from_pairs(unsigned* bitmap, const int* hist_ptr, const int64_t* hist_items, int hb, int he,
                                                       int u0, int B, int i0, int tid) {
  for (int p = hb + tid; p < he; p += NT) {
    const int64_t it = hist_items[p];
    if (it >= i0 && it < i0 + TILE_M) {
      const int lo = hist_owner(hist_ptr, p, u0, min(B, u0 + USERS) - 1);
      const int il = (int)(it - i0);
      atomicOr(&bitmap[(lo - u0) * (TILE_M / 32) + (il >> 5)], 1u << (il & 31));
    }
  }
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
