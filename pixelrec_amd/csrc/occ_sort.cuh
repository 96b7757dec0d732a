// occ_sort.cuh -- the occurrence sort in front of the segment sums of the table gradient (embed_grad.hip): the (<= 3*B*L) row
// occurrences of a step -> keys (one table row id per occurrence) -> stable LSD radix sort of (key, occurrence id) -> the unique
// ids in ascending order (uniq_idx, *n_uniq; id 0 = padding_idx dropped) and the segments of the sorted order (seg_start).  Two
// sorts give the same order: one launch per wide radix pass + one for the segments up to FP_MAX_N occurrences (fused_sort), the
// multi-launch sort above (sort_and_segment).  sort_occurrences is the one place that chooses between them.
//
// Everything is launched with worst-case grids and reads the device-side counts, so the sequence is hipGraph-capturable and needs
// no host synchronisation.
#pragma once
#include "pxr_common.h"

#include <cstdlib>

namespace pxr {

// what an occurrence is.  The sorts know two key derivations: MODE_ROWS (one id per occurrence; MODE_POOL sorts like it) and
// MODE_SASREC (the three uses of the table under an OccLayout); the segment sums (embed_grad.hip) resolve all three.
enum { MODE_ROWS = 0, MODE_SASREC = 1, MODE_POOL = 2 };

constexpr int RS_THREADS = 256;
constexpr int RS_ITEMS = 8;
constexpr int RS_TILE = RS_THREADS * RS_ITEMS;  // 2048 keys per block

// ------------------------------------------------------------------------------------------------ keys
// id layout of the three occurrence kinds: position t of sequence b reads items[b*bstride + off[kind] + t].  SASRec's shifted
// [B, 2, L+1] windows: bstride 2(L+1), off (0, 1, L+2); BERT4Rec's aligned [B, 3, L] planes: bstride 3L, off (0, L, 2L)
struct OccLayout { int64_t bstride, off_in, off_pos, off_neg; };
static inline bool occ_layout_ok(int L, const OccLayout& lay) {
  return lay.off_in >= 0 && lay.off_in + L <= lay.bstride && pxr_bpr_layout_ok(L, lay.bstride, lay.off_pos, lay.off_neg);
}

struct FusedPassArgs {
  const int64_t* src;          // pass 0: idx[n] (MODE_ROWS) or items [B,2,L+1] (MODE_SASREC); later passes: unused
  const int* keys_in; const int* vals_in;
  int* keys_out; int* vals_out;
  int n, B, L, shift, bits, first;
  int64_t n_table;
  OccLayout lay;               // MODE_SASREC: where the three occurrence kinds sit in `src`
  int32_t* status;             // MODE_SASREC: bad-index flag or null
};

// The key of occurrence o.  An id outside [0, n_table) is an error in the reference (nn.Embedding raises on the whole items
// tensor): under MODE_SASREC it sets the bad-index bit of `status` (when given) and is then dropped like padding -- not
// checked_id's rule: a bad id becomes key 0, "dropped", not the nearer end of the table.  The plain (MODE_ROWS) keys only drop.
// flag: this call is the one read of occurrence o that reports an id outside the table (pass 0 of the fused sort reads every key
// once per block for the histogram, and once more, in its own block only, to rank it)
template <int MODE>
__device__ __forceinline__ int occ_key(const FusedPassArgs& a, int o, bool flag = false) {
  int64_t id;
  if constexpr (MODE == 0) {
    id = a.src[o];
  } else {
    const int T = a.B * a.L;
    const int type = o / T, r = o - type * T;
    const int b = r / a.L, t = r - b * a.L;
    const int64_t* row = a.src + (int64_t)b * a.lay.bstride;
    id = row[(type == 0 ? a.lay.off_in : (type == 1 ? a.lay.off_pos : a.lay.off_neg)) + t];
  }
  if (id < 0 || id >= a.n_table) {
    if (MODE != 0 && flag && a.status) atomicOr(a.status, PXR_STATUS_BAD_INDEX);
    return 0;
  }
  return (int)id;
}

// the keys of the multi-launch sort: (keys_out, vals_out)[o] = (occ_key(o), o); of `a`, the source fields, n and the outputs count
template <int MODE>
__global__ void __launch_bounds__(256) occ_keys_kernel(FusedPassArgs a) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= a.n) return;
  a.keys_out[o] = occ_key<MODE>(a, o, true);
  a.vals_out[o] = o;
}

// Rank of this lane's key among the keys one wave ranks in a row, in (call, lane) order within its digit: the ballots find the
// lanes that share the digit `dg` (BITS wide), the lowest of them bumps the wave's counter mycnt[dg] by their number and hands
// the old count to the others.  Every lane of the wave calls it.
template <int BITS>
__device__ __forceinline__ int wave_digit_rank(int dg, bool valid, volatile int* mycnt) {
  const int lane = threadIdx.x & 63;
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (int bit = 0; bit < BITS; ++bit) {
    const bool one = (dg >> bit) & 1;
    const unsigned long long bm = __ballot(one);
    m &= one ? bm : ~bm;
  }
  const int r = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
  int b0 = 0;
  if (valid && r == 0) {  // lowest lane of each digit group bumps this wave's counter
    b0 = mycnt[dg];
    mycnt[dg] = b0 + __popcll(m);
  }
  const int leader = valid ? (__ffsll((long long)m) - 1) : lane;
  b0 = __shfl(b0, leader, 64);
  const int rank = b0 + r;
  __builtin_amdgcn_wave_barrier();
  return rank;
}

// ------------------------------------------------------------------------------------------------ radix sort
__global__ void __launch_bounds__(RS_THREADS) rs_hist_kernel(const int* __restrict__ keys, int n, int shift, int nblk,
                                                             int* __restrict__ hist) {
  __shared__ int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int base = blockIdx.x * RS_TILE;
#pragma unroll
  for (int e = 0; e < RS_ITEMS; ++e) {
    const int i = base + e * RS_THREADS + threadIdx.x;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255], 1);
  }
  __syncthreads();
  hist[threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];  // digit-major so one exclusive scan gives global bases
}

// single-block exclusive scan of `len` ints (len <= 1024 * 256), in place; optionally writes the total
__global__ void __launch_bounds__(1024) scan_excl_kernel(int* __restrict__ data, int len, int* __restrict__ total) {
  __shared__ int wsum[16];
  __shared__ int carry;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (len + 1023) / 1024;
  const int b0 = min(len, tid * per), b1 = min(len, b0 + per);
  int s = 0;
  for (int i = b0; i < b1; ++i) s += data[i];
  // exclusive scan of the 1024 per-thread sums
  const int incl = wave_scan_incl(s);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  if (tid == 0) {
    int c = 0;
    for (int w = 0; w < 16; ++w) { const int t = wsum[w]; wsum[w] = c; c += t; }
    carry = c;
  }
  __syncthreads();
  int run = wsum[wave] + incl - s;
  for (int i = b0; i < b1; ++i) { const int t = data[i]; data[i] = run; run += t; }
  if (total && tid == 0) *total = carry;
}

__global__ void __launch_bounds__(RS_THREADS) rs_scatter_kernel(const int* __restrict__ keys_in,
                                                                const int* __restrict__ vals_in, int n, int shift,
                                                                int nblk, const int* __restrict__ hist_scanned,
                                                                int* __restrict__ keys_out, int* __restrict__ vals_out) {
  __shared__ int wcnt[4][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0;
  __syncthreads();
  const int base = blockIdx.x * RS_TILE + wave * (64 * RS_ITEMS);
  int key[RS_ITEMS], val[RS_ITEMS], rank[RS_ITEMS];
#pragma unroll
  for (int e = 0; e < RS_ITEMS; ++e) {
    const int i = base + e * 64 + lane;   // original order inside the block = (wave, e, lane): ranks keep it => stable
    const bool valid = i < n;
    key[e] = valid ? keys_in[i] : 0;
    val[e] = valid ? vals_in[i] : 0;
    rank[e] = wave_digit_rank<8>((key[e] >> shift) & 255, valid, wcnt[wave]);
  }
  __syncthreads();
  // digit `tid`: exclusive prefix over the 4 waves + this block's global base
  {
    const int g = hist_scanned[tid * nblk + blockIdx.x];
    int c = g;
    for (int w = 0; w < 4; ++w) { const int t = wcnt[w][tid]; wcnt[w][tid] = c; c += t; }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < RS_ITEMS; ++e) {
    const int i = base + e * 64 + lane;
    if (i < n) {
      const int dg = (key[e] >> shift) & 255;
      const int pos = wcnt[wave][dg] + rank[e];
      keys_out[pos] = key[e];
      vals_out[pos] = val[e];
    }
  }
}

// ------------------------------------------------------------------------------------------------ segments
// position i of the sorted keys opens a segment: its key is not the dropped key 0 and differs from the key before it
__device__ __forceinline__ bool seg_head(const int* __restrict__ keys, int i) {
  const int k = keys[i];
  return k != 0 && (i == 0 || keys[i - 1] != k);
}

// per-block head counts
__global__ void __launch_bounds__(RS_THREADS) seg_count_kernel(const int* __restrict__ keys, int n,
                                                               int* __restrict__ blk_count) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const int base = blockIdx.x * RS_TILE + threadIdx.x * RS_ITEMS;
  int c = 0;
#pragma unroll
  for (int e = 0; e < RS_ITEMS; ++e) {
    const int i = base + e;
    if (i < n) c += seg_head(keys, i) ? 1 : 0;
  }
  c = (int)wave_sum((float)c);  // <= 512 per wave: exact in fp32
  if ((threadIdx.x & 63) == 0) atomicAdd(&cnt, c);
  __syncthreads();
  if (threadIdx.x == 0) blk_count[blockIdx.x] = cnt;
}

// assigns unique ids in key order; writes uniq_idx, seg_start (and the end sentinel seg_start[n_uniq] = n)
__global__ void __launch_bounds__(RS_THREADS) seg_assign_kernel(const int* __restrict__ keys, int n,
                                                                const int* __restrict__ blk_off,
                                                                const int* __restrict__ n_uniq,
                                                                int64_t* __restrict__ uniq_idx,
                                                                int* __restrict__ seg_start) {
  __shared__ int wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int base = blockIdx.x * RS_TILE + tid * RS_ITEMS;
  int flag[RS_ITEMS], c = 0;
#pragma unroll
  for (int e = 0; e < RS_ITEMS; ++e) {
    const int i = base + e;
    flag[e] = (i < n && seg_head(keys, i)) ? 1 : 0;
    c += flag[e];
  }
  const int incl = wave_scan_incl(c);
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int woff = 0;
  for (int w = 0; w < wave; ++w) woff += wsum[w];
  int u = blk_off[blockIdx.x] + woff + incl - c;
#pragma unroll
  for (int e = 0; e < RS_ITEMS; ++e) {
    if (flag[e]) {
      uniq_idx[u] = keys[base + e];
      seg_start[u] = base + e;
      ++u;
    }
  }
  if (blockIdx.x == 0 && tid == 0) seg_start[*n_uniq] = n;
}

// ------------------------------------------------------------------------------------------------ fused passes
// For the batch sizes of the training step (n = 3*B*L = 9600 occurrences at B=64) the multi-launch sort above is
// pure launch latency: 13 kernels of ~5 us.  Below, ONE launch per radix pass and ONE for the segments: instead of
// exchanging per-block histograms through global memory (hist -> scan -> scatter), every block redundantly
// histograms ALL n keys in LDS (n is small; the keys sit in L2), which gives it the global digit bases AND the
// counts of the blocks before it without any inter-block communication.  Digits widen to up to 10 bits, so 19-bit
// ids (N = 400 K) need 2 passes.  Same stable order as the multi-launch path => identical results.
constexpr int FP_MAXBITS = 10;
constexpr int FP_BINS = 1 << FP_MAXBITS;
constexpr int FP_THREADS = 1024;         // 16 waves: the redundant histogram is one global round trip for n <= 16 K
constexpr int FP_WAVES = FP_THREADS / 64;
constexpr int FP_ITEMS = 2;              // keys ranked per thread => the same 2048-key tile as the multi-launch path
constexpr int FP_HB = 16;                // keys per thread per histogram batch
constexpr int FP_MAX_N = 32 * RS_TILE;   // beyond this the redundant histogram stops paying
static_assert(FP_THREADS * FP_ITEMS == RS_TILE, "fused passes share the tile size (and workspace) of the radix sort");

template <int MODE>
__global__ void __launch_bounds__(FP_THREADS) fused_pass_kernel(FusedPassArgs a) {
  __shared__ int h_all[FP_BINS];       // histogram of all keys -> exclusive digit bases (+ blocks before this one)
  __shared__ int h_prev[FP_BINS];      // histogram of the keys that belong to earlier blocks
  __shared__ int wcnt[FP_WAVES][FP_BINS];
  __shared__ int wsum[FP_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = 1 << a.bits, mask = nb - 1;
  for (int i = tid; i < nb; i += FP_THREADS) { h_all[i] = 0; h_prev[i] = 0; }
  for (int i = tid; i < FP_WAVES * FP_BINS; i += FP_THREADS) (&wcnt[0][0])[i] = 0;
  __syncthreads();
  const int my0 = blockIdx.x * RS_TILE;
  // FP_HB keys per thread are loaded before the first LDS atomic (one global round trip per 16 K keys); a wave
  // whose 64 keys share one digit (runs of padding zeros, a popular item) adds once instead of 64 times
  for (int i0 = 0; i0 < a.n; i0 += FP_HB * FP_THREADS) {
    int k[FP_HB];
#pragma unroll
    for (int e = 0; e < FP_HB; ++e) {
      const int i = i0 + e * FP_THREADS + tid;
      k[e] = (i < a.n) ? (a.first ? occ_key<MODE>(a, i) : a.keys_in[i]) : -1;
    }
#pragma unroll
    for (int e = 0; e < FP_HB; ++e) {
      const int i = i0 + e * FP_THREADS + tid;          // a wave covers 64 consecutive i: `i < my0` is wave-uniform
      const bool valid = k[e] >= 0;
      const int dg = (k[e] >> a.shift) & mask;
      const int dg0 = __shfl(dg, 0, 64);
      if (__ballot(valid && dg == dg0) == ~0ull) {
        if (lane == 0) { atomicAdd(&h_all[dg], 64); if (i < my0) atomicAdd(&h_prev[dg], 64); }
      } else if (valid) {
        atomicAdd(&h_all[dg], 1);
        if (i < my0) atomicAdd(&h_prev[dg], 1);
      }
    }
  }
  __syncthreads();
  // exclusive scan of h_all over the digits (one bin per thread)
  {
    const int own = (tid < nb) ? h_all[tid] : 0;
    const int incl = wave_scan_incl(own);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int run = incl - own;
    for (int w = 0; w < wave; ++w) run += wsum[w];
    if (tid < nb) h_all[tid] = run + h_prev[tid];
  }
  // rank this block's keys: order inside the block = (wave, e, lane) = ascending index => stable
  volatile int* mycnt = wcnt[wave];
  const int base = my0 + wave * (64 * FP_ITEMS);
  int key[FP_ITEMS], val[FP_ITEMS], rank[FP_ITEMS];
#pragma unroll
  for (int e = 0; e < FP_ITEMS; ++e) {
    const int i = base + e * 64 + lane;
    const bool valid = i < a.n;
    key[e] = valid ? (a.first ? occ_key<MODE>(a, i, true) : a.keys_in[i]) : 0;
    val[e] = valid ? (a.first ? i : a.vals_in[i]) : 0;
    // wave_digit_rank<FP_MAXBITS>, spelled out: called through the helper, the compiler commutes the operands of the ballot ANDs,
    // and the code of this kernel, which every training step runs, is pinned byte for byte (profiles/occ_sort)
    const int dg = (key[e] >> a.shift) & mask;
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < FP_MAXBITS; ++bit) {   // bits above the digit width are 0 in every lane: no-ops
      const bool one = (dg >> bit) & 1;
      const unsigned long long bm = __ballot(one);
      m &= one ? bm : ~bm;
    }
    const int r = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
    int b0 = 0;
    if (valid && r == 0) {  // lowest lane of each digit group bumps this wave's counter
      b0 = mycnt[dg];
      mycnt[dg] = b0 + __popcll(m);
    }
    const int leader = valid ? (__ffsll((long long)m) - 1) : lane;
    b0 = __shfl(b0, leader, 64);
    rank[e] = b0 + r;
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  if (tid < nb) {   // digit tid: exclusive prefix over the waves + global base of this block
    int c = h_all[tid];
    for (int w = 0; w < FP_WAVES; ++w) { const int t = wcnt[w][tid]; wcnt[w][tid] = c; c += t; }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < FP_ITEMS; ++e) {
    const int i = base + e * 64 + lane;
    if (i < a.n) {
      const int pos = wcnt[wave][(key[e] >> a.shift) & mask] + rank[e];
      a.keys_out[pos] = key[e];
      a.vals_out[pos] = val[e];
    }
  }
}

// seg_count + scan + seg_assign in one launch: block b also counts the heads of the tiles before it
__global__ void __launch_bounds__(RS_THREADS) fused_segments_kernel(const int* __restrict__ keys, int n,
                                                                    int64_t* __restrict__ uniq_idx,
                                                                    int* __restrict__ seg_start,
                                                                    int* __restrict__ n_uniq) {
  __shared__ int wsum[4];
  __shared__ int s_prev;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int my0 = blockIdx.x * RS_TILE;
  int cprev = 0;
  for (int i0 = 0; i0 < my0; i0 += 8 * RS_THREADS) {   // my0 is a multiple of 2048 = 8 * 256: no tail
    int k0[8], k1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {                       // all 16 loads in flight before the first compare
      const int i = i0 + e * RS_THREADS + tid;
      k0[e] = keys[i];
      k1[e] = i > 0 ? keys[i - 1] : 0;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {                       // seg_head on the loaded pair (spelled out: see fused_pass_kernel)
      const int i = i0 + e * RS_THREADS + tid;
      cprev += (k0[e] != 0 && (i == 0 || k1[e] != k0[e])) ? 1 : 0;
    }
  }
  cprev = (int)wave_sum((float)cprev);   // < 2^24: exact in fp32
  if (lane == 0) wsum[wave] = cprev;
  __syncthreads();
  if (tid == 0) s_prev = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  const int base = my0 + tid * RS_ITEMS;
  int flag[RS_ITEMS], c = 0;
#pragma unroll
  for (int e = 0; e < RS_ITEMS; ++e) {
    const int i = base + e;
    flag[e] = (i < n) ? (seg_head(keys, i) ? 1 : 0) : 0;
    c += flag[e];
  }
  const int incl = wave_scan_incl(c);
  __syncthreads();
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int woff = 0, tot = 0;
  for (int w = 0; w < 4; ++w) { if (w < wave) woff += wsum[w]; tot += wsum[w]; }
  int u = s_prev + woff + incl - c;
#pragma unroll
  for (int e = 0; e < RS_ITEMS; ++e) {
    if (flag[e]) {
      uniq_idx[u] = keys[base + e];
      seg_start[u] = base + e;
      ++u;
    }
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) {
    *n_uniq = s_prev + tot;
    seg_start[s_prev + tot] = n;
  }
}

}  // namespace pxr

// ------------------------------------------------------------------------------------------------ host side
namespace pxr {

static inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// The sort's workspace: two ping-pong (keys, vals) pairs, the multi-launch sort's histograms and block counts, the segments.
struct SortWs {
  int *keysA, *keysB, *valsA, *valsB, *hist, *blk, *seg_start;
  int nblk;
};
static int64_t carve(void* ws, int n, SortWs* out) {
  const int nblk = (n + RS_TILE - 1) / RS_TILE;
  char* p = (char*)ws;
  int64_t off = 0;
  auto take = [&](int64_t bytes) { char* r = p ? p + off : nullptr; off += align256(bytes); return r; };
  int* kA = (int*)take((int64_t)n * 4); int* kB = (int*)take((int64_t)n * 4);
  int* vA = (int*)take((int64_t)n * 4); int* vB = (int*)take((int64_t)n * 4);
  int* hist = (int*)take((int64_t)256 * nblk * 4);
  int* blk = (int*)take((int64_t)(nblk + 1) * 4);
  int* seg = (int*)take((int64_t)(n + 1) * 4);
  if (out) { out->keysA = kA; out->keysB = kB; out->valsA = vA; out->valsB = vB; out->hist = hist; out->blk = blk;
             out->seg_start = seg; out->nblk = nblk; }
  return off;
}
// carve for entry point `who`, which was handed ws_bytes
static int carve_checked(const char* who, const void* ws, int64_t ws_bytes, int n, SortWs* out) {
  if (carve(const_cast<void*>(ws), n, out) > ws_bytes) { pxr_set_error("%s: workspace too small", who); return PXR_ERR_WORKSPACE; }
  return PXR_OK;
}

// bits of the largest key: ids lie in [0, n_table)
static int id_bits(int64_t n_table) {
  int bits = 1;
  while (((int64_t)1 << bits) < n_table) ++bits;
  return bits;
}
static int radix_passes(int64_t n_table) { return (id_bits(n_table) + 7) / 8; }
static int fused_passes(int64_t n_table) { return (id_bits(n_table) + FP_MAXBITS - 1) / FP_MAXBITS; }
// n <= FP_MAX_N: one launch per (wide) radix pass + one for the segments (PXR_FUSED_SORT=0 forces the multi-launch
// path, for A/B tests)
static bool use_fused_sort(int n) {
  static const int enabled = getenv("PXR_FUSED_SORT") ? atoi(getenv("PXR_FUSED_SORT")) : 1;
  return enabled && n <= FP_MAX_N;
}
// The buffer of `w` in which the sort of n occurrences over n_table ids leaves the sorted occurrence ids: known without
// running it, so phase 2 of a two-phase entry finds them (pxr_seq_occ_sort -> pxr_sasrec_occ_segsum) and a caller can plan
// its use of the other pair (dense_grad in embed_grad.hip)
static const int* final_vals_buffer(const SortWs& w, int n, int64_t n_table) {
  const int npass = use_fused_sort(n) ? fused_passes(n_table) : radix_passes(n_table);
  return (npass & 1) ? w.valsB : w.valsA;   // the ping-pong buffers swap once per pass
}

// the multi-launch sort of the (keys, vals) in pair A of `w`
static int sort_and_segment(SortWs& w, int n, int64_t n_table, int64_t* uniq_idx, int* n_uniq, hipStream_t st,
                            const int** sorted_vals) {
  const int npass = radix_passes(n_table);
  if (256 * w.nblk > 1024 * 256) { pxr_set_error("embed grad: too many occurrences (%d)", n); return PXR_ERR_BAD_ARG; }
  int *kin = w.keysA, *kout = w.keysB, *vin = w.valsA, *vout = w.valsB;
  for (int p = 0; p < npass; ++p) {
    hipLaunchKernelGGL(rs_hist_kernel, dim3(w.nblk), dim3(RS_THREADS), 0, st, kin, n, p * 8, w.nblk, w.hist);
    hipLaunchKernelGGL(scan_excl_kernel, dim3(1), dim3(1024), 0, st, w.hist, 256 * w.nblk, (int*)nullptr);
    hipLaunchKernelGGL(rs_scatter_kernel, dim3(w.nblk), dim3(RS_THREADS), 0, st, kin, vin, n, p * 8, w.nblk, w.hist,
                       kout, vout);
    int* t = kin; kin = kout; kout = t;
    t = vin; vin = vout; vout = t;
  }
  hipLaunchKernelGGL(seg_count_kernel, dim3(w.nblk), dim3(RS_THREADS), 0, st, kin, n, w.blk);
  hipLaunchKernelGGL(scan_excl_kernel, dim3(1), dim3(1024), 0, st, w.blk, w.nblk, n_uniq);
  hipLaunchKernelGGL(seg_assign_kernel, dim3(w.nblk), dim3(RS_THREADS), 0, st, kin, n, w.blk, n_uniq, uniq_idx,
                     w.seg_start);
  *sorted_vals = vin;
  return pxr_check_launch("embed grad (sort/segment)");
}

// the fused sort: `key` holds the source fields (occ_key); pass 0 derives the keys itself
template <int MODE>
static int fused_sort(FusedPassArgs key, const SortWs& w, int64_t* uniq_idx, int* n_uniq, hipStream_t st, const int** sorted_vals) {
  const int bits = id_bits(key.n_table), npass = fused_passes(key.n_table);
  const int width = (bits + npass - 1) / npass;
  int *kin = w.keysA, *kout = w.keysB, *vin = w.valsA, *vout = w.valsB;
  for (int p = 0; p < npass; ++p) {
    FusedPassArgs a = key;
    a.keys_in = kin; a.vals_in = vin; a.keys_out = kout; a.vals_out = vout;
    a.shift = p * width; a.bits = width; a.first = (p == 0);
    hipLaunchKernelGGL(fused_pass_kernel<MODE>, dim3(w.nblk), dim3(FP_THREADS), 0, st, a);
    int* t = kin; kin = kout; kout = t;
    t = vin; vin = vout; vout = t;
  }
  hipLaunchKernelGGL(fused_segments_kernel, dim3(w.nblk), dim3(RS_THREADS), 0, st, kin, key.n, uniq_idx, w.seg_start,
                     n_uniq);
  *sorted_vals = vin;
  return pxr_check_launch("embed grad (fused sort/segment)");
}

// Occurrence keys -> stable sort -> unique ids + segments, for entry point `who`.  SORT == MODE_ROWS: src is idx [n];
// SORT == MODE_SASREC: src is items under (B, L, lay), n = 3 B L, and an id outside the table sets the bad-index bit of the
// status word.  Leaves uniq_idx [<= n] ascending, *n_uniq, w.seg_start and the sorted occurrence ids in *sorted_vals, which is
// final_vals_buffer(w, n, n_table) -- checked here, for both sorts, because later phases rely on it.
template <int SORT>
static int sort_occurrences(const char* who, const int64_t* src, int n, int B, int L, const OccLayout& lay, int64_t n_table,
                            SortWs& w, int64_t* uniq_idx, int* n_uniq, hipStream_t st, const int** sorted_vals) {
  static_assert(SORT == MODE_ROWS || SORT == MODE_SASREC, "the sorts that exist: plain row keys, or the three sequence occurrence kinds");
  FusedPassArgs key{};
  key.src = src; key.n = n; key.B = B; key.L = L; key.n_table = n_table; key.lay = lay;
  key.status = SORT == MODE_SASREC ? pxr_status_word() : nullptr;
  int rc;
  if (use_fused_sort(n)) {
    rc = fused_sort<SORT>(key, w, uniq_idx, n_uniq, st, sorted_vals);
  } else {
    key.keys_out = w.keysA; key.vals_out = w.valsA;
    hipLaunchKernelGGL(occ_keys_kernel<SORT>, dim3((n + 255) / 256), dim3(256), 0, st, key);
    rc = sort_and_segment(w, n, n_table, uniq_idx, n_uniq, st, sorted_vals);
  }
  if (rc) return rc;
  if (*sorted_vals != final_vals_buffer(w, n, n_table)) { pxr_set_error("%s: internal buffer parity", who); return PXR_ERR_LAUNCH; }
  return PXR_OK;
}

}  // namespace pxr
