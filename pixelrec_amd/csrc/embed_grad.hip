// embed_grad.hip -- gradient of the item-embedding table in SPARSE form (K1' of SURVEY.md §2.1).
//
// The reference's nn.Embedding (sasrec.py:31, no sparse=True) makes autograd materialise a dense [N, D] gradient
// (819 MB at N=400K, D=512: zero-fill + scatter-add, `embedding_dense_backward`) that DDP then all-reduces.
// Here the gradient is never dense: the (<= 3*B*L) row occurrences of a step are de-duplicated into
//     uniq_idx[n_uniq] (ascending item ids, id 0 = padding_idx dropped)   and   uniq_rows[n_uniq, D]
// by a stable LSD radix sort of the occurrence ids followed by a segmented sum in occurrence order, so the
// result is bit-reproducible (no float atomics) and identical on every rank given identical inputs.
//
// Occurrences (what autograd would scatter-add):
//   MODE_ROWS   : occurrence o adds  rows[o, :]                       to table row idx[o]   (plain embedding bwd); into sparse
//        rows (pxr_embed_grad_rows_f32) or, over a batch-local row space, into a dense block (pxr_embed_grad_dense_f32: MODIN)
//   MODE_SASREC : the three uses of the table in SASRec.forward (sasrec.py:68-74,88-89), T = B*L, r = o % T:
//        o in [0,T)    input  id items[b,0,t]     adds  dx0[r,:]                 (grad of the LN'd input)
//        o in [T,2T)   target id items[b,0,t+1]   adds  +coef[r] * out[r,:]      (d pos_score)
//        o in [2T,3T)  negative id items[b,1,t+1] adds  -coef[r] * out[r,:]      (d neg_score)
//     which never materialises the [B,2,L+1,D] gather nor its gradient.  The ids sit wherever the caller's layout says
//     (pxr_seq_occ_sort).  Sinks: sparse rows (pxr_sasrec_occ_segsum[_split]), the lazy row update (pxr_sasrec_occ_segsum_apply),
//     or, over a batch-local row space, a dense block (pxr_seq_occ_dense_f32: MOBERT4Rec, each image encoded once).
//   MODE_POOL   : the pooled-history pair models (pool.hip), idx [B*L + 2B] = history rows | target rows, T = B*L, one COMPACT
//        gradient block G [3B, D] (one row per sample for its whole history, one per target):
//        o in [0,T)      history position (b, l) = o / L, o % L   adds  w[b] * G[b,:]     (the pooling weight of sample b)
//        o in [T,T+2B)   target j = o - T                         adds  G[B + j,:]
//     so the L copies of a sample's history gradient are never written out.  The same sums land either in sparse rows
//     (pxr_pool_table_grad_f32) or in a dense [n_rows, D] block over a batch-local row space (pxr_pool_dense_grad_f32: the "table"
//     is the visual encoder's output of the batch, whose gradient autograd takes dense).
//
// Everything is launched with worst-case grids and reads the device-side counts, so the sequence is
// hipGraph-capturable and needs no host synchronisation.
#include "adam_row.cuh"
#include "pxr_common.h"
#include "reduce_multi.cuh"

#include <cstdlib>

namespace pxr {

constexpr int RS_THREADS = 256;
constexpr int RS_ITEMS = 8;
constexpr int RS_TILE = RS_THREADS * RS_ITEMS;  // 2048 keys per block

// ------------------------------------------------------------------------------------------------ keys
__global__ void __launch_bounds__(256) occ_keys_rows_kernel(const int64_t* __restrict__ idx, int n,
                                                            int* __restrict__ keys, int* __restrict__ vals,
                                                            int64_t n_table) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= n) return;
  int64_t r = idx[o];
  if (r < 0 || r >= n_table) r = 0;  // out-of-range ids are dropped like padding
  keys[o] = (int)r;
  vals[o] = o;
}
// id layout of the three occurrence kinds: position t of sequence b reads items[b*bstride + off[kind] + t].  SASRec's shifted
// [B, 2, L+1] windows: bstride 2(L+1), off (0, 1, L+2); BERT4Rec's aligned [B, 3, L] planes: bstride 3L, off (0, L, 2L)
struct OccLayout { int64_t bstride, off_in, off_pos, off_neg; };

// An id outside [0, n_table) is an error in the reference (nn.Embedding raises on the whole items tensor): it sets the bad-index
// bit of `status` (when given) and is then dropped like padding.  The plain (MODE_ROWS) keys only drop.
__global__ void __launch_bounds__(256) occ_keys_sasrec_kernel(const int64_t* __restrict__ items, int B, int L,
                                                              int* __restrict__ keys, int* __restrict__ vals,
                                                              int64_t n_table, OccLayout lay, int32_t* status) {
  const int T = B * L;
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= 3 * T) return;
  const int type = o / T, r = o - type * T;
  const int b = r / L, t = r - b * L;
  const int64_t* row = items + (int64_t)b * lay.bstride;
  int64_t id = row[(type == 0 ? lay.off_in : (type == 1 ? lay.off_pos : lay.off_neg)) + t];
  if (id < 0 || id >= n_table) {   // not checked_id's rule: a bad id becomes key 0, "dropped", not the nearer end of the table
    if (status) atomicOr(status, PXR_STATUS_BAD_INDEX);
    id = 0;
  }
  keys[o] = (int)id;
  vals[o] = o;
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
  int incl = s;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
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
  volatile int* mycnt = wcnt[wave];
  const int base = blockIdx.x * RS_TILE + wave * (64 * RS_ITEMS);
  int key[RS_ITEMS], val[RS_ITEMS], rank[RS_ITEMS];
  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
  for (int e = 0; e < RS_ITEMS; ++e) {
    const int i = base + e * 64 + lane;   // original order inside the block = (wave, e, lane): ranks keep it => stable
    const bool valid = i < n;
    key[e] = valid ? keys_in[i] : 0;
    val[e] = valid ? vals_in[i] : 0;
    const int dg = (key[e] >> shift) & 255;
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (dg >> bit) & 1;
      const unsigned long long bm = __ballot(one);
      m &= one ? bm : ~bm;
    }
    const int r = __popcll(m & lt);
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
// head(i) = key[i] != 0 && (i == 0 || key[i] != key[i-1]);  per-block head counts
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
    if (i < n) {
      const int k = keys[i];
      c += (k != 0 && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
    }
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
  int flag[RS_ITEMS], k[RS_ITEMS];
  int c = 0;
#pragma unroll
  for (int e = 0; e < RS_ITEMS; ++e) {
    const int i = base + e;
    k[e] = (i < n) ? keys[i] : 0;
    flag[e] = (i < n && k[e] != 0 && (i == 0 || keys[i - 1] != k[e])) ? 1 : 0;
    c += flag[e];
  }
  int incl = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int woff = 0;
  for (int w = 0; w < wave; ++w) woff += wsum[w];
  int u = blk_off[blockIdx.x] + woff + incl - c;
#pragma unroll
  for (int e = 0; e < RS_ITEMS; ++e) {
    if (flag[e]) {
      uniq_idx[u] = k[e];
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

struct FusedPassArgs {
  const int64_t* src;          // pass 0: idx[n] (MODE_ROWS) or items [B,2,L+1] (MODE_SASREC); later passes: unused
  const int* keys_in; const int* vals_in;
  int* keys_out; int* vals_out;
  int n, B, L, shift, bits, first;
  int64_t n_table;
  OccLayout lay;               // MODE_SASREC: where the three occurrence kinds sit in `src`
  int32_t* status;             // MODE_SASREC: bad-index flag (occ_keys_sasrec_kernel) or null
};

// flag: this call is the one read of occurrence o that reports an id outside the table (pass 0 reads every key once per block
// for the histogram, and once more, in its own block only, to rank it)
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
    int incl = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
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
  auto head = [&](int i) { const int k = keys[i]; return (k != 0 && (i == 0 || keys[i - 1] != k)) ? 1 : 0; };
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
    for (int e = 0; e < 8; ++e) {
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
    flag[e] = (i < n) ? head(i) : 0;
    c += flag[e];
  }
  int incl = c;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off, 64);
    if (lane >= off) incl += t;
  }
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

// ------------------------------------------------------------------------------------------------ segmented sum
enum { MODE_ROWS = 0, MODE_SASREC = 1, MODE_POOL = 2 };

struct SegSumArgs {
  const int* vals;         // sorted occurrence ids
  const int* seg_start;    // [n_uniq + 1]
  const int* n_uniq;
  const float* src0;       // MODE_ROWS: rows [n, D];  MODE_SASREC: dx0 [T, D];  MODE_POOL: G [3B, D]
  const float* src1;       // MODE_SASREC: out [T, D]
  const float* coef;       // MODE_SASREC: [T];  MODE_POOL: w [B]
  float* uniq_rows;        // [n_uniq, D]
  float scale;             // applied to the summed row (1/world_size for gradient averaging; 1 otherwise)
  int D, T;
  // segments of more than `split` occurrences (0: none) are LEFT OUT by segsum_kernel, which lists them in big_rows (any order;
  // big_count is the caller-zeroed cursor): segsum_parts_kernel / segsum_big_kernel sum them on many workgroups
  int split;
  int* big_count;          // [0] cursor, [1] the count as the parts kernel saw it
  int* big_rows;           // [big_cap]
  float* partials;         // [max_parts, D]
  int big_cap;
  // MODE_POOL is never split, so its history length L (T = B * L) takes max_parts' place: the argument block, and with it every
  // kernel of the other modes, keeps the layout it had before this mode existed
  union { int max_parts; int L; };
};

// 512 threads = G = 512/dv groups of dv threads (dv = D/4 float4 columns; D = 512: 4 groups of 128).
//  * Short segments (<= SEG_SHORT occurrences -- almost every row: the negatives and the tail of the Zipf
//    popularity): each GROUP sums one unique row on its own -- resolves the occurrences, has all their row loads
//    in flight at once and adds them in occurrence order.  No LDS, no barrier: the latency chain is
//    seg_start -> sorted ids -> rows, and a workgroup retires G rows per pass.
//  * Long segments (a popular item: hundreds of occurrences): all G groups cooperate on the row -- per chunk of
//    <= 512 occurrences the (source row, coefficient) pairs are resolved into LDS, group g adds occurrences g, g+G,
//    ... with 8 row loads in flight, and the G partial rows are combined in group order through LDS.
// Both are fixed summation orders => bit-reproducible.
constexpr int SEG_THREADS = 512;
constexpr int SEG_CHUNK = 512;   // occurrences staged per pass (long segments)
constexpr int SEG_SHORT = 8;     // longest segment a single group handles

template <int MODE>
__device__ __forceinline__ void seg_resolve(const SegSumArgs& a, int o, int64_t& off, float& cf) {
  if constexpr (MODE == MODE_ROWS) {
    off = (int64_t)o * a.D;
    cf = 1.f;
  } else if constexpr (MODE == MODE_POOL) {
    const int b = o / a.L;                                      // only meaningful for o < T
    off = (int64_t)(o < a.T ? b : a.T / a.L + (o - a.T)) * a.D;
    cf = o < a.T ? a.coef[b] : 1.f;
  } else {
    const int type = o / a.T, r = o - type * a.T;
    // type 0 reads src0 (dx0); types 1/2 read src1 (out): the source is encoded in the sign bit of the offset
    off = (type == 0) ? (int64_t)r * a.D : ~((int64_t)r * a.D);
    cf = (type == 0) ? 1.f : (type == 1 ? a.coef[r] : -a.coef[r]);
  }
}
template <int MODE>
__device__ __forceinline__ const float* seg_row(const SegSumArgs& a, int64_t off) {
  if constexpr (MODE == MODE_SASREC) return off >= 0 ? a.src0 + off : a.src1 + ~off;
  else return a.src0 + off;
}

constexpr int SEG_EPOCH = 16;    // passes between two looks at the long rows (no barrier inside an epoch)

// What the segment sums do with a finished row sum is a SINK, so that the summation below exists once:
//   SegStoreRows : uniq_rows[u,:] = scale * sum -- the table gradient as sparse rows, for an exchange or a later row update;
//   SegApplyRows : the lazy AdamW step of table row uniq_idx[u] with the sum as its gradient (adam_row.cuh), for a row that is
//                  current through the step before; nothing is written to uniq_rows.
//   SegStoreDense: d_rows[uniq_idx[u],:] = sum -- the gradient as a dense block whose other rows the entry point has zeroed;
//                  nothing is written to uniq_rows.
// kRowId: the sink needs the row's id (row_id) and not only its rank u among the unique rows.
// A sink names the row (row_id), reads what it needs of it as soon as the row is known (begin: the loads then travel under the
// occurrence loads instead of behind them), takes the sum of one float4 column (finish) and, once EVERY lane of the row has
// called begin, closes the row from one lane (mark).
struct SegStoreRows {
  static constexpr bool kApply = false, kRowId = false;
  struct Row {};
  __device__ __forceinline__ void init() {}
  __device__ __forceinline__ int row_id(int) const { return 0; }
  __device__ __forceinline__ Row begin(int, int) const { return Row{}; }
  __device__ __forceinline__ void finish(const SegSumArgs& a, const Row&, int u, int col, float4 acc) const {
    acc.x *= a.scale; acc.y *= a.scale; acc.z *= a.scale; acc.w *= a.scale;
    *reinterpret_cast<float4*>(a.uniq_rows + (int64_t)u * a.D + col) = acc;
  }
  __device__ __forceinline__ bool closes(const Row&) const { return false; }
  __device__ __forceinline__ void mark(int) const {}
};

struct SegApplyRows {
  static constexpr bool kApply = true, kRowId = true;
  float* p; float* m; float* v; int* last;
  const int64_t* uniq_idx;       // [n_uniq] table row of unique id u (0: padding, skipped like a row outside the table)
  int64_t n_table;               // rows of p / m / v / last
  const float4* hyper;           // per-step scalars (adamw.hip): the step applied is entry t_prev + 1
  const int64_t* step_dev;       // optional: t_prev = *step_dev (completed steps)
  int t_prev, D;
  AdamConsts c;
  int32_t* status;               // PXR_STATUS_ROWS_STALE: a row that was not current through t_prev was left untouched
  AdamHyper h;                   // (init)
  struct Row { float4 p, m, v; int64_t o; int last; bool ok; };
  __device__ __forceinline__ void init() {
    if (step_dev) t_prev = (int)step_dev[0];
    h = adam_step_hyper(c, hyper[t_prev + 1]);
  }
  __device__ __forceinline__ int row_id(int u) const { return (int)uniq_idx[u]; }
  // p / m / v of the row's float4 column `col` and last[row]: every lane of the row asks for last[row] (one address per wave)
  __device__ __forceinline__ Row begin(int row, int col) const {
    Row r;
    r.ok = row > 0 && (int64_t)row < n_table;
    r.o = (int64_t)row * D + col;
    r.last = 0;
    r.p = r.m = r.v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r.ok) {
      r.last = last[row];
      r.p = *reinterpret_cast<const float4*>(p + r.o);
      r.m = *reinterpret_cast<const float4*>(m + r.o);
      r.v = *reinterpret_cast<const float4*>(v + r.o);
    }
    return r;
  }
  __device__ __forceinline__ bool closes(const Row& r) const { return r.ok && r.last == t_prev; }
  // the gradient is the plain sum (the entry point serves scale == 1 only)
  __device__ __forceinline__ void finish(const SegSumArgs&, const Row& r, int, int, const float4 acc) const {
    if (!closes(r)) return;          // padding / outside the table: dropped; not current: left as it is (lane_stale flags it)
    float pe[4] = {r.p.x, r.p.y, r.p.z, r.p.w}, me[4] = {r.m.x, r.m.y, r.m.z, r.m.w}, ve[4] = {r.v.x, r.v.y, r.v.z, r.v.w};
    const float ge[4] = {acc.x, acc.y, acc.z, acc.w};
    adam_apply_row<4>(pe, me, ve, ge, h);
    *reinterpret_cast<float4*>(p + r.o) = make_float4(pe[0], pe[1], pe[2], pe[3]);
    *reinterpret_cast<float4*>(m + r.o) = make_float4(me[0], me[1], me[2], me[3]);
    *reinterpret_cast<float4*>(v + r.o) = make_float4(ve[0], ve[1], ve[2], ve[3]);
  }
  // one lane of the row: a row that is in the table but not current raises the status bit
  __device__ __forceinline__ void lane_stale(const Row& r) const {
    if (r.ok && r.last != t_prev && status) atomicOr(status, PXR_STATUS_ROWS_STALE);
  }
  __device__ __forceinline__ void mark(int row) const { adam_row_mark(last, row, t_prev + 1); }
};

struct SegStoreDense {
  static constexpr bool kApply = false, kRowId = true;
  float* d_rows;                 // [n_rows, D]
  const int64_t* uniq_idx;       // [n_uniq] row of unique id u: in (0, n_rows) by the sort's keys; anything else is dropped
  int64_t n_rows;
  int D;
  struct Row { int64_t o; bool ok; };
  __device__ __forceinline__ void init() {}
  __device__ __forceinline__ int row_id(int u) const { return (int)uniq_idx[u]; }
  __device__ __forceinline__ Row begin(int row, int col) const {
    return Row{(int64_t)row * D + col, row > 0 && (int64_t)row < n_rows};
  }
  // the plain sum: MODE_POOL's scale is 1
  __device__ __forceinline__ void finish(const SegSumArgs&, const Row& r, int, int, const float4 acc) const {
    if (r.ok) *reinterpret_cast<float4*>(d_rows + r.o) = acc;
  }
  __device__ __forceinline__ bool closes(const Row&) const { return false; }
  __device__ __forceinline__ void mark(int) const {}
};

// one unique row summed by the WHOLE workgroup (a long segment, or D too wide for row groups).  Block-uniform call.
template <int MODE, class SINK>
__device__ __forceinline__ void seg_long_row(const SegSumArgs& a, const SINK& sink, int u, int dv, int G, int g, int c0, bool active,
                                             float4* sred, int64_t* s_off, float* s_cf) {
  const int s0 = a.seg_start[u], s1 = a.seg_start[u + 1];
  const int row = (SINK::kRowId && g == 0) ? sink.row_id(u) : 0;
  bool close = false;
  for (int cb = 0; cb < dv; cb += SEG_THREADS) {  // dv > 512 (D > 2048): column blocks
    const int c4 = cb + c0;
    // the sink's loads of the row are asked for before the occurrences: they arrive under the chunk loop.  Every lane that
    // will finish a column has read the row's state before the first barrier below, so the closing store after the last
    // column cannot be seen by a lane that has not looked yet
    typename SINK::Row r{};
    if (g == 0 && c4 < dv) r = sink.begin(row, c4 * 4);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int sb = s0; sb < s1; sb += SEG_CHUNK) {
      const int cnt = min(SEG_CHUNK, s1 - sb);
      __syncthreads();
      for (int j = threadIdx.x; j < cnt; j += SEG_THREADS) seg_resolve<MODE>(a, a.vals[sb + j], s_off[j], s_cf[j]);
      __syncthreads();
      if (active && c4 < dv) {
        int j = g;
        for (; j + 7 * G < cnt; j += 8 * G) {
          float4 v[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] = *reinterpret_cast<const float4*>(seg_row<MODE>(a, s_off[j + q * G]) + c4 * 4);
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const float cf = s_cf[j + q * G];
            acc.x += cf * v[q].x; acc.y += cf * v[q].y; acc.z += cf * v[q].z; acc.w += cf * v[q].w;
          }
        }
        for (; j < cnt; j += G) {
          const float cf = s_cf[j];
          const float4 v = *reinterpret_cast<const float4*>(seg_row<MODE>(a, s_off[j]) + c4 * 4);
          acc.x += cf * v.x; acc.y += cf * v.y; acc.z += cf * v.z; acc.w += cf * v.w;
        }
      }
    }
    if (G > 1) {
      __syncthreads();
      if (active) sred[g * dv + c0] = acc;
      __syncthreads();
      if (g == 0) {
        for (int k = 1; k < G; ++k) {
          const float4 t = sred[k * dv + c0];
          acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
        }
      }
    }
    if (g == 0 && c4 < dv) {
      sink.finish(a, r, u, c4 * 4, acc);
      if constexpr (SINK::kApply) {
        if (threadIdx.x == 0 && cb == 0) { close = sink.closes(r); sink.lane_stale(r); }
      }
    }
  }
  if constexpr (SINK::kApply) {
    if (close) sink.mark(row);       // thread 0, behind at least one barrier that every reader of the row's state has passed
  }
}

// The short path is a chain of three dependent loads (seg_start -> sorted ids -> coefficient and row) of which only the last
// moves data: round 5 keeps the first two links of the NEXT two passes in flight while the rows of this pass are summed (the
// segment bounds two passes ahead, the first two ids one pass ahead), and looks at the long rows once per SEG_EPOCH passes instead
// of synchronising the eight waves twice per pass.  Same sums in the same order.  The body of segsum_kernel and of
// segsum_apply_kernel: they differ in the sink alone.  nblk: the workgroups that run it, blocks [0, nblk) of the grid (a launch
// that carries a rider has more blocks than that: segsum_rider below).
template <int MODE, class SINK>
__device__ __forceinline__ void segsum_body(const SegSumArgs& a, SINK sink, const int nblk) {
  extern __shared__ __attribute__((aligned(16))) float4 sred[];  // [G][dv]
  __shared__ int64_t s_off[SEG_CHUNK];
  __shared__ float s_cf[SEG_CHUNK];
  __shared__ int s_longrow[SEG_EPOCH * (SEG_THREADS / 64)];
  // apply sink: the rows a group closed in this epoch.  A row's lanes are several waves that no barrier holds together inside an
  // epoch, so the store that marks the row as updated waits for the epoch's barrier: no lane then still has to read the mark
  __shared__ int s_close[SINK::kApply ? SEG_EPOCH * (SEG_THREADS / 64) : 1];
  sink.init();
  const int nu = *a.n_uniq;
  const int dv = a.D >> 2;
  const bool wide = dv > SEG_THREADS;                 // D > 2048: one row per workgroup, column blocks
  const int G = wide ? 1 : SEG_THREADS / dv;          // <= 8 for D >= 256
  const int g = wide ? 0 : threadIdx.x / dv;
  const int c0 = wide ? threadIdx.x : threadIdx.x - g * dv;
  const bool active = g < G;
  if (wide || G > SEG_THREADS / 64) {                 // one row per pass, the whole workgroup on it
    for (int u = blockIdx.x; u < nu; u += nblk) {
      seg_long_row<MODE>(a, sink, u, dv, G, g, c0, active, sred, s_off, s_cf);
      __syncthreads();
    }
    return;
  }
  const int stride = nblk * G;
  auto bounds = [&](int u, int& s0, int& cnt, int& row) {
    s0 = 0; cnt = 0; row = 0;
    if (active && u < nu) {
      s0 = a.seg_start[u]; cnt = a.seg_start[u + 1] - s0;
      if constexpr (SINK::kRowId) row = sink.row_id(u);
    }
  };
  auto first_ids = [&](int s0, int cnt, int& i0, int& i1) {
    i0 = 0; i1 = 0;
    if (cnt > 0 && cnt <= SEG_SHORT) { i0 = a.vals[s0]; if (cnt > 1) i1 = a.vals[s0 + 1]; }
  };
  int base = blockIdx.x * G;
  int s0C, cntC, rowC, i0C, i1C, s0B, cntB, rowB;
  bounds(base + g, s0C, cntC, rowC);
  first_ids(s0C, cntC, i0C, i1C);
  bounds(base + stride + g, s0B, cntB, rowB);
  while (base < nu) {                                  // block-uniform
    int e = 0;
    for (; e < SEG_EPOCH && base < nu; ++e, base += stride) {
      const int u = base + g;
      int s0A, cntA, rowA, i0B, i1B;
      bounds(u + 2 * stride, s0A, cntA, rowA);         // two passes ahead
      first_ids(s0B, cntB, i0B, i1B);                  // one pass ahead
      int longrow = -1, closed = -1;
      if (active && u < nu) {
        if (cntC > SEG_SHORT) {
          longrow = u;
        } else {
          const typename SINK::Row r = sink.begin(rowC, c0 * 4);
          float4 v[SEG_SHORT];
          float cf[SEG_SHORT];
#pragma unroll
          for (int j = 0; j < SEG_SHORT; ++j) {
            cf[j] = 0.f;
            v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < cntC) {
              const int o = j == 0 ? i0C : (j == 1 ? i1C : a.vals[s0C + j]);
              int64_t off;
              seg_resolve<MODE>(a, o, off, cf[j]);
              v[j] = *reinterpret_cast<const float4*>(seg_row<MODE>(a, off) + c0 * 4);
            }
          }
          float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int j = 0; j < SEG_SHORT; ++j)
            if (j < cntC) { acc.x += cf[j] * v[j].x; acc.y += cf[j] * v[j].y; acc.z += cf[j] * v[j].z; acc.w += cf[j] * v[j].w; }
          sink.finish(a, r, u, c0 * 4, acc);
          if constexpr (SINK::kApply) {
            if (c0 == 0) { if (sink.closes(r)) closed = rowC; sink.lane_stale(r); }
          }
        }
      }
      if (active && c0 == 0) {
        s_longrow[e * G + g] = longrow;
        if constexpr (SINK::kApply) s_close[e * G + g] = closed;
      }
      s0C = s0B; cntC = cntB; rowC = rowB; i0C = i0B; i1C = i1B; s0B = s0A; cntB = cntA; rowB = rowA;
    }
    __syncthreads();
    if constexpr (SINK::kApply) {
      if ((int)threadIdx.x < e * G && s_close[threadIdx.x] >= 0) sink.mark(s_close[threadIdx.x]);
    }
    for (int q = 0; q < e * G; ++q) {
      const int u = s_longrow[q];                      // block-uniform
      if (u < 0) continue;
      if (a.split > 0 && a.seg_start[u + 1] - a.seg_start[u] > a.split) {
        if (threadIdx.x == 0) {
          const int slot = atomicAdd(a.big_count, 1);  // <= n / split such rows exist: big_cap covers them all
          if (slot < a.big_cap) a.big_rows[slot] = u;
        }
        continue;
      }
      seg_long_row<MODE>(a, sink, u, dv, G, g, c0, active, sred, s_off, s_cf);
    }
    __syncthreads();                                   // s_longrow is rewritten by the next epoch
  }
}

// ---- the tail rider (reduce_multi.cuh) -----------------------------------------------------------------------------------
// The single phase-2 launch of a step may carry the small reductions that close the backward pass (LayerNorm dgamma|dbeta, bias
// and position column sums, the dropout counter bump, the loss sum): blocks [0, seg_grid) are the segment sums, unchanged;
// blocks [seg_grid, seg_grid + r.blocks) run the rider and nothing else.  The branch is block-uniform and comes first.  The two
// kinds of block share no byte (the launch sites say which buffers are whose), so there is nothing to order between them: no
// atomics on data, no fences, no flags.  A rider block borrows the dynamic LDS of the carrier (sred, SEG_THREADS * 16 bytes).
static_assert(PXR_RIDER_THREADS == SEG_THREADS, "a rider block has the carrier's shape");
static_assert(PXR_RIDER_LDS <= SEG_THREADS * 16, "a rider block fits the carrier's dynamic LDS");
// true: this block was a rider block and is done.  seg_grid: the carrier's block count
__device__ __forceinline__ bool segsum_rider(const TailRider& r, int& seg_grid) {
  extern __shared__ __attribute__((aligned(16))) float4 sred[];
  seg_grid = (int)gridDim.x - r.blocks;
  if (r.blocks == 0 || (int)blockIdx.x < seg_grid) return false;
  pxr_tail_rider_block(r, (int)blockIdx.x - seg_grid, sred);
  return true;
}

template <int MODE>
__global__ void __launch_bounds__(SEG_THREADS) segsum_kernel(SegSumArgs a, TailRider r) {
  int seg_grid;
  if (segsum_rider(r, seg_grid)) return;
  segsum_body<MODE>(a, SegStoreRows{}, seg_grid);
}

// The segment sums with the row update done where the sum is formed: no uniq_rows store, no second launch reading it back.
// split must be 0 (every segment is summed here).
__global__ void __launch_bounds__(SEG_THREADS) segsum_apply_kernel(SegSumArgs a, SegApplyRows s, TailRider r) {
  int seg_grid;
  if (segsum_rider(r, seg_grid)) return;
  segsum_body<MODE_SASREC>(a, s, seg_grid);
}

// +0.0 over the dense block in front of its segment sums (a kernel, not a memset node: h2.hip's h2_zero_kernel says why)
__global__ void __launch_bounds__(256) dense_zero_kernel(float4* __restrict__ p, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// MODE's segment sums into a dense block (SegStoreDense): the sums and their order are segsum_kernel<MODE>'s (MODE_POOL: the
// pooled pair models' compact block; MODE_ROWS: one gradient row per occurrence; MODE_SASREC: the sequence models' three terms).
template <int MODE>
__global__ void __launch_bounds__(SEG_THREADS) segsum_dense_kernel(SegSumArgs a, SegStoreDense s) {
  segsum_body<MODE>(a, s, (int)gridDim.x);
}

// ---- very long segments on many workgroups (round 5) --------------------------------------------------------------------------
// A Zipf-popular item of a big batch has thousands of occurrences (B = 2 048: 13 000 for the first rank, 27 MB of source rows), and
// one workgroup streams ~70 GB/s: its row alone took 400-600 us of the 640 us launch while the rest of the chip was done after
// 250.  Rows of more than SEG_SPLIT occurrences are therefore cut into parts of SEG_CHUNK occurrences, each part summed by its
// own workgroup exactly as seg_long_row sums a chunk (G group sums combined in group order) into a partial row, and the partial
// rows of a row are added in part order: a fixed order again, whatever the order in which segsum_kernel listed the rows.
constexpr int SEG_SPLIT = 1024;
constexpr int SEG_BIG_MAX = 2048;    // rows the LDS prefix table holds: n <= SEG_SPLIT * SEG_BIG_MAX occurrences (2 M)

// first[i] = index of row i's first part (exclusive prefix of ceil(cnt / SEG_CHUNK)); returns the total.  All threads call it.
__device__ __forceinline__ int seg_big_prefix(const SegSumArgs& a, int nb, int* first) {
  __syncthreads();
  for (int i = threadIdx.x; i < nb; i += SEG_THREADS) {
    const int u = a.big_rows[i];
    first[i + 1] = (a.seg_start[u + 1] - a.seg_start[u] + SEG_CHUNK - 1) / SEG_CHUNK;
  }
  __syncthreads();
  if (threadIdx.x == 0) {               // <= 2 048 LDS adds
    int run = 0;
    for (int i = 0; i < nb; ++i) { const int c = first[i + 1]; first[i] = run; run += c; }
    first[nb] = run;
  }
  __syncthreads();
  return first[nb];
}

template <int MODE>
__global__ void __launch_bounds__(SEG_THREADS) segsum_parts_kernel(SegSumArgs a) {
  extern __shared__ __attribute__((aligned(16))) float4 sred[];  // [G][dv]
  __shared__ int64_t s_off[SEG_CHUNK];
  __shared__ float s_cf[SEG_CHUNK];
  __shared__ int s_first[SEG_BIG_MAX + 1];
  const int nb = min(a.big_count[0], a.big_cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) a.big_count[1] = nb;     // segsum_big_kernel resets the cursor: it reads this copy
  if (nb == 0) return;
  const int dv = a.D >> 2, G = SEG_THREADS / dv, g = threadIdx.x / dv, c0 = threadIdx.x - g * dv;
  const bool active = g < G;
  const int total = min(seg_big_prefix(a, nb, s_first), a.max_parts);
  for (int p = blockIdx.x; p < total; p += gridDim.x) {
    int lo = 0, hi = nb - 1;                           // the row whose parts include p
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_first[mid] <= p) lo = mid; else hi = mid - 1; }
    const int u = a.big_rows[lo];
    const int sb = a.seg_start[u] + (p - s_first[lo]) * SEG_CHUNK;
    const int cnt = min(SEG_CHUNK, a.seg_start[u + 1] - sb);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    for (int j = threadIdx.x; j < cnt; j += SEG_THREADS) seg_resolve<MODE>(a, a.vals[sb + j], s_off[j], s_cf[j]);
    __syncthreads();
    if (active) {
      int j = g;
      for (; j + 7 * G < cnt; j += 8 * G) {
        float4 v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = *reinterpret_cast<const float4*>(seg_row<MODE>(a, s_off[j + q * G]) + c0 * 4);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const float cf = s_cf[j + q * G];
          acc.x += cf * v[q].x; acc.y += cf * v[q].y; acc.z += cf * v[q].z; acc.w += cf * v[q].w;
        }
      }
      for (; j < cnt; j += G) {
        const float cf = s_cf[j];
        const float4 v = *reinterpret_cast<const float4*>(seg_row<MODE>(a, s_off[j]) + c0 * 4);
        acc.x += cf * v.x; acc.y += cf * v.y; acc.z += cf * v.z; acc.w += cf * v.w;
      }
    }
    __syncthreads();
    if (active) sred[g * dv + c0] = acc;
    __syncthreads();
    if (g == 0) {
      for (int k = 1; k < G; ++k) {
        const float4 t = sred[k * dv + c0];
        acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
      }
      *reinterpret_cast<float4*>(a.partials + (int64_t)p * a.D + c0 * 4) = acc;
    }
  }
}

// uniq_rows[u] = scale * (partial 0 + partial 1 + ...) for the listed rows; leaves the cursor at zero for the next call
__global__ void __launch_bounds__(SEG_THREADS) segsum_big_kernel(SegSumArgs a) {
  __shared__ int s_first[SEG_BIG_MAX + 1];
  const int nb = a.big_count[1];
  if (blockIdx.x == 0 && threadIdx.x == 0) a.big_count[0] = 0;
  if (nb == 0) return;
  const int dv = a.D >> 2;
  const int total = seg_big_prefix(a, nb, s_first);
  const int rows_per_wg = SEG_THREADS / dv, g = threadIdx.x / dv, c0 = threadIdx.x - g * dv;
  for (int i = blockIdx.x * rows_per_wg + g; i < nb; i += gridDim.x * rows_per_wg) {
    if (g >= rows_per_wg) break;
    const int p0 = s_first[i], p1 = min(s_first[i + 1], a.max_parts);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = p0; p < p1; ++p) {
      const float4 t = *reinterpret_cast<const float4*>(a.partials + (int64_t)p * a.D + c0 * 4);
      acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
    }
    acc.x *= a.scale; acc.y *= a.scale; acc.z *= a.scale; acc.w *= a.scale;
    *reinterpret_cast<float4*>(a.uniq_rows + (int64_t)a.big_rows[i] * a.D + c0 * 4) = acc;
  }
  (void)total;
}

static inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

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

static int sort_and_segment(SortWs& w, int n, int64_t n_table, int64_t* uniq_idx, int* n_uniq, hipStream_t st,
                            const int** sorted_vals) {
  int bits = 1;
  while (((int64_t)1 << bits) < n_table) ++bits;
  const int npass = (bits + 7) / 8;
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

// ------------------------------------------------------------------------------------------------ rank merge
// Data-parallel merge of W rank-local sparse gradients that are each ALREADY sorted and unique (the output of the
// kernels above), concatenated as idx_all [W, cap] / rows_all [W, cap, D]; every list is ascending over its whole
// `cap` (unused tail slots hold ids >= n_table).  No second sort: a lower-bound search finds where an id sits in
// the other W-1 lists, the lowest rank holding an id owns its output slot and adds the other ranks' rows in rank
// order -- a fixed order that is the same on every replica, so replicas stay bit-identical.  The output is NOT
// compacted: slot e = (rank, i) carries (id, summed row) if that rank owns the id, else id 0 (= padding_idx, which
// every consumer skips); *n_out = W * cap.
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

static int radix_passes(int64_t n_table) {
  int bits = 1;
  while (((int64_t)1 << bits) < n_table) ++bits;
  return (bits + 7) / 8;
}
// n <= FP_MAX_N: one launch per (wide) radix pass + one for the segments (PXR_FUSED_SORT=0 forces the multi-launch
// path, for A/B tests).  Returns the buffer the sorted occurrence ids end up in through *sorted_vals.
static bool use_fused_sort(int n) {
  static const int enabled = getenv("PXR_FUSED_SORT") ? atoi(getenv("PXR_FUSED_SORT")) : 1;
  return enabled && n <= FP_MAX_N;
}
static int fused_passes(int64_t n_table) {
  int bits = 1;
  while (((int64_t)1 << bits) < n_table) ++bits;
  return (bits + FP_MAXBITS - 1) / FP_MAXBITS;
}
template <int MODE>
static int fused_sort(const int64_t* src, int n, int B, int L, int64_t n_table, const SortWs& w, int64_t* uniq_idx,
                      int* n_uniq, hipStream_t st, const int** sorted_vals, OccLayout lay = OccLayout{}) {
  int bits = 1;
  while (((int64_t)1 << bits) < n_table) ++bits;
  const int npass = fused_passes(n_table);
  const int width = (bits + npass - 1) / npass;
  int *kin = w.keysA, *kout = w.keysB, *vin = w.valsA, *vout = w.valsB;
  for (int p = 0; p < npass; ++p) {
    FusedPassArgs a{};
    a.src = src; a.keys_in = kin; a.vals_in = vin; a.keys_out = kout; a.vals_out = vout;
    a.n = n; a.B = B; a.L = L; a.shift = p * width; a.bits = width; a.first = (p == 0); a.n_table = n_table; a.lay = lay;
    a.status = MODE == MODE_SASREC ? pxr_status_word() : nullptr;
    hipLaunchKernelGGL(fused_pass_kernel<MODE>, dim3(w.nblk), dim3(FP_THREADS), 0, st, a);
    int* t = kin; kin = kout; kout = t;
    t = vin; vin = vout; vout = t;
  }
  hipLaunchKernelGGL(fused_segments_kernel, dim3(w.nblk), dim3(RS_THREADS), 0, st, kin, n, uniq_idx, w.seg_start,
                     n_uniq);
  *sorted_vals = vin;
  return pxr_check_launch("embed grad (fused sort/segment)");
}
// where pxr_seq_occ_sort leaves the sorted occurrence ids for pxr_sasrec_occ_segsum
static const int* sasrec_sorted_vals(const SortWs& w, int n, int64_t n_table) {
  const int npass = use_fused_sort(n) ? fused_passes(n_table) : radix_passes(n_table);
  return (npass & 1) ? w.valsB : w.valsA;   // the ping-pong buffers swap once per pass
}

extern "C" int64_t pxr_embed_grad_ws_bytes(int64_t n_occ) {
  return carve(nullptr, (int)n_occ, nullptr);
}

// Plain embedding backward in sparse form: (idx[n], rows[n, D]) -> (uniq_idx[<=n] ascending, uniq_rows, *n_uniq).
// idx == 0 (padding_idx) and out-of-range ids are dropped.  uniq_idx/uniq_rows must hold n entries / rows.
extern "C" int pxr_embed_grad_rows_f32(const int64_t* idx, int64_t n, const float* rows, int D, int64_t n_table,
                                       float scale, int64_t* uniq_idx, float* uniq_rows, int32_t* n_uniq_dev, void* ws,
                                       int64_t ws_bytes, void* stream) {
  PXR_REQUIRE(idx && rows && uniq_idx && uniq_rows && n_uniq_dev && ws, "pxr_embed_grad_rows_f32: null pointer");
  PXR_REQUIRE(n > 0 && n < (1ll << 30) && D > 0 && D % 4 == 0 && n_table > 0 && n_table < (1ll << 31),
              "pxr_embed_grad_rows_f32: bad shape");
  SortWs w;
  if (carve(ws, (int)n, &w) > ws_bytes) { pxr_set_error("pxr_embed_grad_rows_f32: workspace too small"); return PXR_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  const int* sorted_vals = nullptr;
  int rc;
  if (use_fused_sort((int)n)) {
    rc = fused_sort<MODE_ROWS>(idx, (int)n, 0, 0, n_table, w, uniq_idx, n_uniq_dev, st, &sorted_vals);
  } else {
    hipLaunchKernelGGL(occ_keys_rows_kernel, dim3(((int)n + 255) / 256), dim3(256), 0, st, idx, (int)n, w.keysA,
                       w.valsA, n_table);
    rc = sort_and_segment(w, (int)n, n_table, uniq_idx, n_uniq_dev, st, &sorted_vals);
  }
  if (rc) return rc;
  SegSumArgs a{};
  a.vals = sorted_vals; a.seg_start = w.seg_start; a.n_uniq = n_uniq_dev; a.src0 = rows; a.uniq_rows = uniq_rows;
  a.scale = scale; a.D = D; a.T = (int)n;
  const int grid = (int)(n < 4096 ? n : 4096);
  hipLaunchKernelGGL(segsum_kernel<MODE_ROWS>, dim3(grid), dim3(SEG_THREADS), SEG_THREADS * 16, st, a, TailRider{});
  return pxr_check_launch("pxr_embed_grad_rows_f32");
}

// The table gradient of the pooled-history pair models (pool.hip) without one gradient row per occurrence: gidx [B L + 2 B] (the
// row every occurrence's gradient goes to, 0 = padding: dropped) is sorted exactly as pxr_embed_grad_rows_f32 sorts its idx, and
// the segment sum resolves occurrence o to (G row o / L, w[o / L]) for o < B L and to (G row B + (o - B L), 1) beyond (MODE_POOL).
extern "C" int pxr_pool_table_grad_f32(const int64_t* gidx, int B, int L, const float* G, const float* w, int D, int64_t n_table,
                                       int64_t* uniq_idx, float* uniq_rows, int32_t* n_uniq_dev, void* ws, int64_t ws_bytes,
                                       void* stream) {
  PXR_REQUIRE(gidx && G && w && uniq_idx && uniq_rows && n_uniq_dev && ws, "pxr_pool_table_grad_f32: null pointer");
  PXR_REQUIRE(B > 0 && L >= 1 && (int64_t)B * (L + 2) < (1ll << 30) && D > 0 && D % 4 == 0 && D <= 4096 && n_table > 0 &&
              n_table < (1ll << 31), "pxr_pool_table_grad_f32: bad shape (B=%d, L=%d, D=%d)", B, L, D);
  PXR_REQUIRE((((uintptr_t)G | (uintptr_t)uniq_rows) & 15) == 0, "pxr_pool_table_grad_f32: G and uniq_rows must be 16-byte aligned");
  PXR_REQUIRE(G != uniq_rows, "pxr_pool_table_grad_f32: uniq_rows must not alias G");
  const int n = B * (L + 2);
  SortWs sw;
  if (carve(ws, n, &sw) > ws_bytes) { pxr_set_error("pxr_pool_table_grad_f32: workspace too small"); return PXR_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  const int* sorted_vals = nullptr;
  int rc;
  if (use_fused_sort(n)) {
    rc = fused_sort<MODE_ROWS>(gidx, n, 0, 0, n_table, sw, uniq_idx, n_uniq_dev, st, &sorted_vals);
  } else {
    hipLaunchKernelGGL(occ_keys_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, st, gidx, n, sw.keysA, sw.valsA, n_table);
    rc = sort_and_segment(sw, n, n_table, uniq_idx, n_uniq_dev, st, &sorted_vals);
  }
  if (rc) return rc;
  SegSumArgs a{};
  a.vals = sorted_vals; a.seg_start = sw.seg_start; a.n_uniq = n_uniq_dev; a.src0 = G; a.coef = w; a.uniq_rows = uniq_rows;
  a.scale = 1.f; a.D = D; a.T = B * L; a.L = L;
  const int grid = n < 4096 ? n : 4096;
  hipLaunchKernelGGL(segsum_kernel<MODE_POOL>, dim3(grid), dim3(SEG_THREADS), SEG_THREADS * 16, st, a, TailRider{});
  return pxr_check_launch("pxr_pool_table_grad_f32");
}

// What the dense entries share: zero d_rows [n_rows, D], sort the n occurrence keys of `src` -- SORT == MODE_ROWS: src is gidx [n],
// sorted exactly as pxr_embed_grad_rows_f32 sorts its idx; SORT == MODE_SASREC: src is items under (B, L, lay), n = 3 B L, sorted
// exactly as pxr_seq_occ_sort sorts them, bad-index bit included -- and run segsum_body<MODE> over `a` (the caller has filled the
// sources) into the dense sink.  The unique-row list the sort needs lives in the workspace: the four key / value buffers are handed
// to the sort as (keysA, valsA | keysB, valsB), so the ping-pong pair that does not hold the final order is one contiguous stretch
// of >= 8 n bytes, and the count takes the spare last entry of the block-count buffer.
template <int MODE, int SORT>
static int dense_grad(const char* who, const int64_t* src, int n, int B, int L, const OccLayout& lay, SegSumArgs a, int64_t n_rows,
                      float* d_rows, void* ws, int64_t ws_bytes, hipStream_t st) {
  static_assert(SORT == MODE_ROWS || SORT == MODE_SASREC, "the sorts that exist: plain row keys, or the three sequence occurrence kinds");
  const int D = a.D;
  SortWs sw;
  if (carve(ws, n, &sw) > ws_bytes) { pxr_set_error("%s: workspace too small", who); return PXR_ERR_WORKSPACE; }
  { int* t = sw.keysB; sw.keysB = sw.valsA; sw.valsA = t; }     // slots (0, 1) = pair A, (2, 3) = pair B
  const int* final_vals = sasrec_sorted_vals(sw, n, n_rows);
  int64_t* uniq_idx = (int64_t*)(final_vals == sw.valsB ? sw.keysA : sw.keysB);
  int32_t* n_uniq_dev = sw.blk + sw.nblk;
  const int64_t n4 = n_rows * (D / 4);
  hipLaunchKernelGGL(dense_zero_kernel, dim3((unsigned)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096)), dim3(256), 0, st, (float4*)d_rows, n4);
  const int* sorted_vals = nullptr;
  int rc;
  if (use_fused_sort(n)) {
    rc = fused_sort<SORT>(src, n, B, L, n_rows, sw, uniq_idx, n_uniq_dev, st, &sorted_vals, lay);
  } else {
    if constexpr (SORT == MODE_SASREC)
      hipLaunchKernelGGL(occ_keys_sasrec_kernel, dim3((n + 255) / 256), dim3(256), 0, st, src, B, L, sw.keysA, sw.valsA, n_rows, lay,
                         pxr_status_word());
    else
      hipLaunchKernelGGL(occ_keys_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, st, src, n, sw.keysA, sw.valsA, n_rows);
    rc = sort_and_segment(sw, n, n_rows, uniq_idx, n_uniq_dev, st, &sorted_vals);
  }
  if (rc) return rc;
  if (sorted_vals != final_vals) { pxr_set_error("%s: internal buffer parity", who); return PXR_ERR_LAUNCH; }
  a.vals = sorted_vals; a.seg_start = sw.seg_start; a.n_uniq = n_uniq_dev;
  SegStoreDense s{};
  s.d_rows = d_rows; s.uniq_idx = uniq_idx; s.n_rows = n_rows; s.D = D;
  const int grid = n < 4096 ? n : 4096;
  hipLaunchKernelGGL(segsum_dense_kernel<MODE>, dim3(grid), dim3(SEG_THREADS), SEG_THREADS * 16, st, a, s);
  return pxr_check_launch(who);
}

// The same gradient as a DENSE block over a batch-local row space (the pixel versions of the pooled pair models: the rows are the
// visual encoder's outputs for the batch's distinct images): d_rows [n_rows, D] gets the segment sum of every referenced row in
// (0, n_rows) -- pxr_pool_table_grad_f32's sums bit for bit (the same sort, segsum_body<MODE_POOL>, another sink) -- and exactly
// +0.0 everywhere else (row 0 and every unreferenced row), whatever it held before: the block is zeroed here, by a launch in front of
// the segment sums on the same stream (dense_grad).
extern "C" int pxr_pool_dense_grad_f32(const int64_t* gidx, int B, int L, const float* G, const float* w, int D, int64_t n_rows,
                                       float* d_rows, void* ws, int64_t ws_bytes, void* stream) {
  PXR_REQUIRE(gidx && G && w && d_rows && ws, "pxr_pool_dense_grad_f32: null pointer");
  PXR_REQUIRE(B > 0 && L >= 1 && (int64_t)B * (L + 2) < (1ll << 30) && D > 0 && D % 4 == 0 && D <= 4096 && n_rows > 0 &&
              n_rows < (1ll << 31), "pxr_pool_dense_grad_f32: bad shape (B=%d, L=%d, D=%d)", B, L, D);
  PXR_REQUIRE((((uintptr_t)G | (uintptr_t)d_rows) & 15) == 0, "pxr_pool_dense_grad_f32: G and d_rows must be 16-byte aligned");
  const char *g0 = (const char*)G, *g1 = g0 + (int64_t)3 * B * D * 4, *d0 = (const char*)d_rows, *d1 = d0 + n_rows * D * 4;
  PXR_REQUIRE(d1 <= g0 || g1 <= d0, "pxr_pool_dense_grad_f32: d_rows must not alias G");
  SegSumArgs a{};
  a.src0 = G; a.coef = w; a.scale = 1.f; a.D = D; a.T = B * L; a.L = L;
  return dense_grad<MODE_POOL, MODE_ROWS>("pxr_pool_dense_grad_f32", gidx, B * (L + 2), 0, 0, OccLayout{}, a, n_rows, d_rows, ws, ws_bytes, (hipStream_t)stream);
}

// pxr_embed_grad_rows_f32's sums (scale 1) as a DENSE block over a batch-local row space (MODIN: DIN's backward leaves one gradient
// row per occurrence, and the rows are the visual encoder's outputs): d_rows [n_rows, D] gets, at every referenced row in
// (0, n_rows), the sparse entry's sum bit for bit -- the same sort, segsum_body<MODE_ROWS>, the dense sink -- and exactly +0.0
// everywhere else, whatever it held before (zeroed here, on the same stream).  idx == 0 and ids outside [0, n_rows) are dropped.
extern "C" int pxr_embed_grad_dense_f32(const int64_t* idx, int64_t n, const float* rows, int D, int64_t n_rows, float* d_rows,
                                        void* ws, int64_t ws_bytes, void* stream) {
  PXR_REQUIRE(idx && rows && d_rows && ws, "pxr_embed_grad_dense_f32: null pointer");
  PXR_REQUIRE(n > 0 && n < (1ll << 30) && D > 0 && D % 4 == 0 && D <= 4096 && n_rows > 0 && n_rows < (1ll << 31),
              "pxr_embed_grad_dense_f32: bad shape (n=%lld, D=%d)", (long long)n, D);
  PXR_REQUIRE((((uintptr_t)rows | (uintptr_t)d_rows) & 15) == 0, "pxr_embed_grad_dense_f32: rows and d_rows must be 16-byte aligned");
  const char *g0 = (const char*)rows, *g1 = g0 + n * D * 4, *d0 = (const char*)d_rows, *d1 = d0 + n_rows * D * 4;
  PXR_REQUIRE(d1 <= g0 || g1 <= d0, "pxr_embed_grad_dense_f32: d_rows must not alias rows");
  SegSumArgs a{};
  a.src0 = rows; a.scale = 1.f; a.D = D; a.T = (int)n;
  return dense_grad<MODE_ROWS, MODE_ROWS>("pxr_embed_grad_dense_f32", idx, (int)n, 0, 0, OccLayout{}, a, n_rows, d_rows, ws, ws_bytes, (hipStream_t)stream);
}

// Phase 1 of the table gradient: occurrence keys -> stable sort -> unique ids + segments.  Depends on `items` only, so it can
// run BEFORE the forward pass (the lazy table optimizer needs the unique rows of the batch to bring them up to date before they
// are read).  The sorted state stays in `ws` for phase 2: the caller must keep `ws` untouched in between.  The three occurrence
// kinds -- input | target | negative of position t of sequence b -- are at items[b*id_bstride + {in_off, pos_off, neg_off} + t]:
// SASRec's shifted [B, 2, L+1] windows are (2(L+1), 0, 1, L+2); BERT4Rec's items [B, 3, L] = masked sequence | original sequence |
// negatives are (3L, 0, L, 2L) -- the table's three uses in reference IDNet/bert4rec.py:76-81,98-111 under autograd; its
// mask-token row is an ordinary row, row 0 (padding_idx) is dropped.  An id outside [0, n_table) is dropped too and sets the
// bad-index bit of the status word (the reference's nn.Embedding raises).  Phase 2 is pxr_sasrec_occ_segsum[_split] whatever the
// layout: the occurrence o of kind k at row r = b*L + t adds dx0[r], +coef[r] out[r] or -coef[r] out[r].
extern "C" int pxr_seq_occ_sort(const int64_t* items, int B, int L, int64_t id_bstride, int64_t in_off, int64_t pos_off,
                                int64_t neg_off, int64_t n_table, int64_t* uniq_idx, int32_t* n_uniq_dev, void* ws,
                                int64_t ws_bytes, void* stream) {
  PXR_REQUIRE(id_bstride > 0 && in_off >= 0 && pos_off >= 0 && neg_off >= 0 && in_off + L <= id_bstride && pos_off + L <= id_bstride &&
              neg_off + L <= id_bstride, "pxr_seq_occ_sort: bad id layout");
  PXR_REQUIRE(items && uniq_idx && n_uniq_dev && ws, "pxr_seq_occ_sort: null pointer");
  const int64_t n64 = (int64_t)3 * B * L;
  PXR_REQUIRE(B > 0 && L > 0 && n64 < (1ll << 30) && n_table > 0 && n_table < (1ll << 31), "pxr_seq_occ_sort: bad shape");
  const int n = (int)n64;
  const OccLayout lay{id_bstride, in_off, pos_off, neg_off};
  SortWs w;
  if (carve(ws, n, &w) > ws_bytes) { pxr_set_error("pxr_seq_occ_sort: workspace too small"); return PXR_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  const int* sorted_vals = nullptr;
  if (use_fused_sort(n)) {
    int rc = fused_sort<MODE_SASREC>(items, n, B, L, n_table, w, uniq_idx, n_uniq_dev, st, &sorted_vals, lay);
    if (rc) return rc;
    if (sorted_vals != sasrec_sorted_vals(w, n, n_table)) { pxr_set_error("pxr_seq_occ_sort: internal buffer parity"); return PXR_ERR_LAUNCH; }
    return PXR_OK;
  }
  hipLaunchKernelGGL(occ_keys_sasrec_kernel, dim3((n + 255) / 256), dim3(256), 0, st, items, B, L, w.keysA, w.valsA,
                     n_table, lay, pxr_status_word());
  int rc = sort_and_segment(w, n, n_table, uniq_idx, n_uniq_dev, st, &sorted_vals);
  if (rc) return rc;
  if (sorted_vals != sasrec_sorted_vals(w, n, n_table)) { pxr_set_error("pxr_seq_occ_sort: internal buffer parity"); return PXR_ERR_LAUNCH; }
  return PXR_OK;
}

// pxr_seq_occ_sort + pxr_sasrec_occ_segsum(scale = 1) in one call with the DENSE sink (MOBERT4Rec: the "table" is E =
// visual_encoder(the batch's distinct images), whose gradient autograd takes dense): d_rows [n_rows, D] gets, at every referenced
// row in (0, n_rows), the row the two phases leave in uniq_rows for that id, bit for bit -- the same keys under the same layout, the
// same sort, segsum_body<MODE_SASREC>, another sink -- and exactly +0.0 everywhere else, whatever it held before (zeroed here, on the
// same stream).  Key 0 and ids outside [0, n_rows) are dropped; the latter set the bad-index bit, as in pxr_seq_occ_sort.
extern "C" int pxr_seq_occ_dense_f32(const int64_t* items, int B, int L, int64_t id_bstride, int64_t in_off, int64_t pos_off,
                                     int64_t neg_off, const float* dx0, const float* out, const float* coef, int D, int64_t n_rows,
                                     float* d_rows, void* ws, int64_t ws_bytes, void* stream) {
  PXR_REQUIRE(id_bstride > 0 && in_off >= 0 && pos_off >= 0 && neg_off >= 0 && in_off + L <= id_bstride && pos_off + L <= id_bstride &&
              neg_off + L <= id_bstride, "pxr_seq_occ_dense_f32: bad id layout");
  PXR_REQUIRE(items && dx0 && out && coef && d_rows && ws, "pxr_seq_occ_dense_f32: null pointer");
  const int64_t n64 = (int64_t)3 * B * L;
  PXR_REQUIRE(B > 0 && L > 0 && n64 < (1ll << 30) && D > 0 && D % 4 == 0 && D <= 4096 && n_rows > 0 && n_rows < (1ll << 31),
              "pxr_seq_occ_dense_f32: bad shape (B=%d, L=%d, D=%d)", B, L, D);
  PXR_REQUIRE((((uintptr_t)dx0 | (uintptr_t)out | (uintptr_t)d_rows) & 15) == 0,
              "pxr_seq_occ_dense_f32: dx0, out and d_rows must be 16-byte aligned");
  const int64_t src_bytes = (int64_t)B * L * D * 4;
  const char *d0 = (const char*)d_rows, *d1 = d0 + n_rows * D * 4;
  PXR_REQUIRE((d1 <= (const char*)dx0 || (const char*)dx0 + src_bytes <= d0) && (d1 <= (const char*)out || (const char*)out + src_bytes <= d0),
              "pxr_seq_occ_dense_f32: d_rows must not alias dx0 or out");
  SegSumArgs a{};
  a.src0 = dx0; a.src1 = out; a.coef = coef; a.scale = 1.f; a.D = D; a.T = B * L;
  return dense_grad<MODE_SASREC, MODE_SASREC>("pxr_seq_occ_dense_f32", items, (int)n64, B, L, OccLayout{id_bstride, in_off, pos_off, neg_off},
                                              a, n_rows, d_rows, ws, ws_bytes, (hipStream_t)stream);
}

// Phase 2: uniq_rows[u,:] = scale * sum over the occurrences of unique id u (see the header comment for the terms).
extern "C" int pxr_sasrec_occ_segsum(const void* ws, int64_t ws_bytes, int B, int L, const float* dx0, const float* out,
                                     const float* coef, int D, int64_t n_table, float scale,
                                     const int32_t* n_uniq_dev, float* uniq_rows, void* stream, const void* rider) {
  PXR_REQUIRE(ws && dx0 && out && coef && n_uniq_dev && uniq_rows, "pxr_sasrec_occ_segsum: null pointer");
  PXR_REQUIRE(B > 0 && L > 0 && D > 0 && D % 4 == 0, "pxr_sasrec_occ_segsum: bad shape");
  const int n = 3 * B * L;
  SortWs w;
  if (carve(const_cast<void*>(ws), n, &w) > ws_bytes) { pxr_set_error("pxr_sasrec_occ_segsum: workspace too small"); return PXR_ERR_WORKSPACE; }
  SegSumArgs a{};
  a.vals = sasrec_sorted_vals(w, n, n_table); a.seg_start = w.seg_start; a.n_uniq = n_uniq_dev; a.src0 = dx0; a.src1 = out;
  a.coef = coef; a.uniq_rows = uniq_rows; a.scale = scale; a.D = D; a.T = B * L;
  const int grid = n < 4096 ? n : 4096;
  TailRider r;
  if (int rc = pxr_tail_rider_prepare(rider, "pxr_sasrec_occ_segsum", &r)) return rc;
  // who touches what (nothing is shared, so the rider blocks need no ordering against the carrier's):
  //   carrier: reads the occurrence workspace ws (sorted ids, segment bounds), n_uniq_dev, dx0, out, coef; writes uniq_rows;
  //   rider:   reads the partial workspaces of the LayerNorm / column-sum first stages and lossrow; writes the slices of the
  //            flat gradient buffer (LN gamma|beta, biases, positions), the dropout step counter and the loss scalar.
  hipLaunchKernelGGL(segsum_kernel<MODE_SASREC>, dim3(grid + r.blocks), dim3(SEG_THREADS), SEG_THREADS * 16, (hipStream_t)stream, a, r);
  return pxr_check_launch("pxr_sasrec_occ_segsum");
}

// Phase 2 with the lazy AdamW row update inside (segsum_apply_kernel): what pxr_sasrec_occ_segsum(scale = 1) followed by
// pxr_adamw_rows_f32(rows = uniq_idx, grows = uniq_rows, t_apply = t_prev + 1) leaves in table / m / v / last for rows that are
// current through t_prev, bit for bit, in one launch and without the round trip of the summed rows through uniq_rows (which is not
// written).  uniq_idx / n_uniq_dev: pxr_seq_occ_sort's output.  hyper: the per-step scalar table (pxr_adamw_hyper_append), entry
// t_prev + 1 must exist.  step_dev != NULL: t_prev = *step_dev (hipGraph-replayable).  A row with last[row] != t_prev is left
// untouched and raises PXR_STATUS_ROWS_STALE; id 0 and ids outside [0, table_rows) are skipped.
extern "C" int pxr_sasrec_occ_segsum_apply(const void* ws, int64_t ws_bytes, int B, int L, const float* dx0, const float* out,
                                           const float* coef, int D, int64_t n_table, const int32_t* n_uniq_dev,
                                           const int64_t* uniq_idx, float* table, float* m, float* v, int32_t* last,
                                           int64_t table_rows, const void* hyper, int64_t t_prev, const int64_t* step_dev,
                                           double beta1, double beta2, double eps, void* stream, const void* rider) {
  PXR_REQUIRE(ws && dx0 && out && coef && n_uniq_dev && uniq_idx && table && m && v && last && hyper,
              "pxr_sasrec_occ_segsum_apply: null pointer");
  PXR_REQUIRE(B > 0 && L > 0 && D > 0 && D % 4 == 0 && D <= 4096, "pxr_sasrec_occ_segsum_apply: bad shape (D <= 4096)");
  PXR_REQUIRE(table_rows > 0 && table_rows < (1ll << 31) && t_prev >= 0 && t_prev < (1ll << 31) - 1,
              "pxr_sasrec_occ_segsum_apply: bad table size / step");
  const int n = 3 * B * L;
  SortWs w;
  if (carve(const_cast<void*>(ws), n, &w) > ws_bytes) { pxr_set_error("pxr_sasrec_occ_segsum_apply: workspace too small"); return PXR_ERR_WORKSPACE; }
  SegSumArgs a{};
  a.vals = sasrec_sorted_vals(w, n, n_table); a.seg_start = w.seg_start; a.n_uniq = n_uniq_dev; a.src0 = dx0; a.src1 = out;
  a.coef = coef; a.scale = 1.f; a.D = D; a.T = B * L;
  SegApplyRows s{};
  s.p = table; s.m = m; s.v = v; s.last = last; s.uniq_idx = uniq_idx; s.n_table = table_rows;
  s.hyper = (const float4*)hyper; s.step_dev = step_dev; s.t_prev = (int)t_prev; s.D = D;
  s.c = AdamConsts{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps};
  s.status = pxr_status_word();
  const int grid = n < 4096 ? n : 4096;
  TailRider r;
  if (int rc = pxr_tail_rider_prepare(rider, "pxr_sasrec_occ_segsum_apply", &r)) return rc;
  // who touches what (nothing is shared, so the rider blocks need no ordering against the carrier's):
  //   carrier: reads the occurrence workspace ws (sorted ids, segment bounds), n_uniq_dev, uniq_idx, dx0, out, coef, the hyper
  //            slot of step t_prev + 1 and the optimizer's step counter step_dev; reads and writes the touched rows of table / m /
  //            v and their last[] marks; may raise the status word;
  //   rider:   reads the partial workspaces of the LayerNorm / column-sum first stages and lossrow; writes the slices of the
  //            flat gradient buffer (LN gamma|beta, biases, positions), the DROPOUT step counter (another word than step_dev: no
  //            segment-sum kernel reads it) and the loss scalar.
  hipLaunchKernelGGL(segsum_apply_kernel, dim3(grid + r.blocks), dim3(SEG_THREADS), SEG_THREADS * 16, (hipStream_t)stream, a, s, r);
  return pxr_check_launch("pxr_sasrec_occ_segsum_apply");
}

// Phase 2 for big batches: the same sums with the rows of more than 1 024 occurrences cut into parts that many workgroups sum
// (segsum_parts_kernel): three launches instead of one, worth it from ~30 000 occurrences (B >= 200 at L = 50).  `ws2`:
// pxr_sasrec_occ_split_ws_bytes(B, L, D) bytes whose first 256 are ZERO at the first call; every call leaves them zero again.
// Bit-reproducible; the long rows' sums are associated differently from pxr_sasrec_occ_segsum's (part by part).
static void split_layout(int n, int D, int* big_cap, int* max_parts, int64_t* off_rows, int64_t* off_part, int64_t* total) {
  *big_cap = n / SEG_SPLIT + 1;
  *max_parts = n / SEG_CHUNK + *big_cap + 1;
  *off_rows = 256;
  *off_part = align256(256 + (int64_t)*big_cap * 4);
  *total = *off_part + (int64_t)*max_parts * D * 4;
}
extern "C" int64_t pxr_sasrec_occ_split_ws_bytes(int B, int L, int D) {
  const int64_t n = (int64_t)3 * B * L;
  if (B <= 0 || L <= 0 || D <= 0 || D % 4 || D / 4 > SEG_THREADS || SEG_THREADS / (D / 4) > SEG_THREADS / 64 ||
      n > (int64_t)SEG_SPLIT * SEG_BIG_MAX) return 0;      // shapes the split kernels do not serve
  int bc, mp; int64_t o1, o2, tot;
  split_layout((int)n, D, &bc, &mp, &o1, &o2, &tot);
  return tot;
}
extern "C" int pxr_sasrec_occ_segsum_split(const void* ws, int64_t ws_bytes, int B, int L, const float* dx0, const float* out,
                                           const float* coef, int D, int64_t n_table, float scale, const int32_t* n_uniq_dev,
                                           float* uniq_rows, void* ws2, int64_t ws2_bytes, void* stream) {
  PXR_REQUIRE(ws && dx0 && out && coef && n_uniq_dev && uniq_rows && ws2, "pxr_sasrec_occ_segsum_split: null pointer");
  PXR_REQUIRE(B > 0 && L > 0 && D > 0 && D % 4 == 0, "pxr_sasrec_occ_segsum_split: bad shape");
  const int64_t need = pxr_sasrec_occ_split_ws_bytes(B, L, D);
  PXR_REQUIRE(need > 0, "pxr_sasrec_occ_segsum_split: shape not served (B=%d, L=%d, D=%d): use pxr_sasrec_occ_segsum", B, L, D);
  if (need > ws2_bytes) { pxr_set_error("pxr_sasrec_occ_segsum_split: second workspace too small"); return PXR_ERR_WORKSPACE; }
  const int n = 3 * B * L;
  SortWs w;
  if (carve(const_cast<void*>(ws), n, &w) > ws_bytes) { pxr_set_error("pxr_sasrec_occ_segsum_split: workspace too small"); return PXR_ERR_WORKSPACE; }
  SegSumArgs a{};
  a.vals = sasrec_sorted_vals(w, n, n_table); a.seg_start = w.seg_start; a.n_uniq = n_uniq_dev; a.src0 = dx0; a.src1 = out;
  a.coef = coef; a.uniq_rows = uniq_rows; a.scale = scale; a.D = D; a.T = B * L;
  int64_t o1, o2, tot;
  split_layout(n, D, &a.big_cap, &a.max_parts, &o1, &o2, &tot);
  a.split = SEG_SPLIT;
  a.big_count = (int*)ws2; a.big_rows = (int*)((char*)ws2 + o1); a.partials = (float*)((char*)ws2 + o2);
  hipStream_t st = (hipStream_t)stream;
  const int grid = n < 4096 ? n : 4096;
  hipLaunchKernelGGL(segsum_kernel<MODE_SASREC>, dim3(grid), dim3(SEG_THREADS), SEG_THREADS * 16, st, a, TailRider{});
  hipLaunchKernelGGL(segsum_parts_kernel<MODE_SASREC>, dim3(a.max_parts < 1024 ? a.max_parts : 1024), dim3(SEG_THREADS), SEG_THREADS * 16, st, a);
  hipLaunchKernelGGL(segsum_big_kernel, dim3(a.big_cap < 64 ? a.big_cap : 64), dim3(SEG_THREADS), 0, st, a);
  return pxr_check_launch("pxr_sasrec_occ_segsum_split");
}

extern "C" int64_t pxr_merge_rows_ws_bytes(int W, int64_t cap) {
  return align256((int64_t)W * cap * W * 4);
}

static int launch_merge(const MergeSrc& src, int W, int64_t cap, int D, int64_t n_table, float scale, int64_t* out_idx,
                        float* out_rows, int32_t* n_out_dev, void* ws, hipStream_t st, const char* what) {
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
  PXR_REQUIRE(W >= 1 && W <= 64 && cap > 0 && (int64_t)W * cap * W < (1ll << 31) && D > 0 && D % 4 == 0 &&
              n_table > 0, "pxr_merge_sorted_rows_f32: bad shape");
  if (pxr_merge_rows_ws_bytes(W, cap) > ws_bytes) { pxr_set_error("pxr_merge_sorted_rows_f32: workspace too small"); return PXR_ERR_WORKSPACE; }
  MergeSrc src{};
  src.ids = (const char*)idx_all;   src.ids_stride = cap * 8;
  src.rows = (const char*)rows_all; src.rows_stride = cap * (int64_t)D * 4;
  return launch_merge(src, W, cap, D, n_table, scale, out_idx, out_rows, n_out_dev, ws, (hipStream_t)stream,
                      "pxr_merge_sorted_rows_f32");
}

// The packed block one rank contributes to a ONE-collective exchange: {int64 ids[cap]; int32 count; zero padding up to a
// 16-byte boundary; float rows[cap][D]}.
extern "C" int64_t pxr_packed_rows_offset(int64_t cap) { return ((cap + 1) * 8 + 15) & ~(int64_t)15; }
extern "C" int64_t pxr_packed_rows_bytes(int64_t cap, int D) { return pxr_packed_rows_offset(cap) + cap * (int64_t)D * 4; }

extern "C" int pxr_merge_packed_rows_f32(const void* packed_all, int W, int64_t cap, int D, int64_t n_table, float scale,
                                         int64_t* out_idx, float* out_rows, int32_t* n_out_dev, void* ws,
                                         int64_t ws_bytes, void* stream) {
  PXR_REQUIRE(packed_all && out_idx && out_rows && n_out_dev && ws, "pxr_merge_packed_rows_f32: null pointer");
  PXR_REQUIRE(W >= 1 && W <= 64 && cap > 0 && (int64_t)W * cap * W < (1ll << 31) && D > 0 && D % 4 == 0 &&
              n_table > 0, "pxr_merge_packed_rows_f32: bad shape");
  PXR_REQUIRE(((uintptr_t)packed_all & 15) == 0, "pxr_merge_packed_rows_f32: packed_all must be 16-byte aligned");
  if (pxr_merge_rows_ws_bytes(W, cap) > ws_bytes) { pxr_set_error("pxr_merge_packed_rows_f32: workspace too small"); return PXR_ERR_WORKSPACE; }
  const int64_t block = pxr_packed_rows_bytes(cap, D);
  MergeSrc src{};
  src.ids = (const char*)packed_all;                                   src.ids_stride = block;
  src.rows = (const char*)packed_all + pxr_packed_rows_offset(cap);    src.rows_stride = block;
  src.counts = (const char*)packed_all + cap * 8;                      src.counts_stride = block;
  return launch_merge(src, W, cap, D, n_table, scale, out_idx, out_rows, n_out_dev, ws, (hipStream_t)stream,
                      "pxr_merge_packed_rows_f32");
}

// The TWO-collective exchange with a reduced row capacity: every rank all-gathers the HEAD of its packed block ({ids[cap],
// count, pad} = pxr_packed_rows_offset(cap) bytes) and only the first `cap_x` rows.  cap_x is a bound on the unique rows
// of a batch that the caller knows (e.g. from the batcher); a count above it sets bit 1 of the status word
// (pxr_set_status_word) -- the host raises -- and the list is cut at cap_x.  Output: W * cap_x slots.
extern "C" int pxr_merge_split_rows_f32(const void* heads_all, const float* rows_all, int W, int64_t cap, int64_t cap_x,
                                        int D, int64_t n_table, float scale, int64_t* out_idx, float* out_rows,
                                        int32_t* n_out_dev, void* ws, int64_t ws_bytes, void* stream) {
  PXR_REQUIRE(heads_all && rows_all && out_idx && out_rows && n_out_dev && ws, "pxr_merge_split_rows_f32: null pointer");
  PXR_REQUIRE(W >= 1 && W <= 64 && cap > 0 && cap_x > 0 && cap_x <= cap && (int64_t)W * cap_x * W < (1ll << 31) && D > 0 &&
              D % 4 == 0 && n_table > 0, "pxr_merge_split_rows_f32: bad shape");
  PXR_REQUIRE((((uintptr_t)heads_all | (uintptr_t)rows_all) & 15) == 0, "pxr_merge_split_rows_f32: unaligned input");
  if (pxr_merge_rows_ws_bytes(W, cap_x) > ws_bytes) { pxr_set_error("pxr_merge_split_rows_f32: workspace too small"); return PXR_ERR_WORKSPACE; }
  const int64_t head = pxr_packed_rows_offset(cap);
  MergeSrc src{};
  src.ids = (const char*)heads_all;               src.ids_stride = head;
  src.counts = (const char*)heads_all + cap * 8;  src.counts_stride = head;
  src.rows = (const char*)rows_all;               src.rows_stride = cap_x * (int64_t)D * 4;
  src.status = pxr_status_word();
  return launch_merge(src, W, cap_x, D, n_table, scale, out_idx, out_rows, n_out_dev, ws, (hipStream_t)stream,
                      "pxr_merge_split_rows_f32");
}

// ---- row-sharded table helpers (BASELINE configs[3]; pixelrec_amd/model/sharded.py) ---------------------------------
// Owner of item id = id % W; its row in the owner's shard = id / W + 1 (local row 0 is an all-zero dummy, so the
// "index 0 = skip / contributes zeros" convention of the gather and AdamW-rows kernels keeps working).
namespace pxr {
__global__ void __launch_bounds__(256) shard_local_rows_kernel(const int64_t* __restrict__ ids, int64_t n, int W, int rank,
                                                               int64_t n_table, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t id = ids[i];
  out[i] = (id > 0 && id < n_table && id % W == rank) ? id / W + 1 : 0;
}
// W ascending id lists of length cap (tail = ids >= n_table): like shard_local_rows, but an id requested by several
// ranks keeps its local row only in the LOWEST-ranked list that contains it -- a duplicate-free work list for the lazy
// AdamW catch-up (two waves replaying the same row concurrently would race on p/m/v/last).
__global__ void __launch_bounds__(256) shard_first_rows_kernel(const int64_t* __restrict__ ids, int W, int cap, int rank,
                                                               int64_t n_table, int64_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)W * cap) return;
  const int64_t id = ids[t];
  int64_t r = 0;
  if (id > 0 && id < n_table && id % W == rank) {
    r = id / W + 1;
    const int q = (int)(t / cap);
    for (int p = 0; p < q && r; ++p) {
      const int64_t* list = ids + (int64_t)p * cap;
      int lo = 0, hi = cap;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < id) lo = mid + 1; else hi = mid;
      }
      if (lo < cap && list[lo] == id) r = 0;
    }
  }
  out[t] = r;
}
// out[i] = 1 + position of ids[i] in the ascending list uniq[0..n_uniq)  (0 for padding / absent ids)
__global__ void __launch_bounds__(256) ids_to_compact_kernel(const int64_t* __restrict__ ids, int64_t n,
                                                             const int64_t* __restrict__ uniq,
                                                             const int32_t* __restrict__ n_uniq,
                                                             int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t id = ids[i];
  int lo = 0, hi = *n_uniq;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (uniq[mid] < id) lo = mid + 1; else hi = mid;
  }
  out[i] = (id > 0 && lo < *n_uniq && uniq[lo] == id) ? lo + 1 : 0;
}
// The hit-row exchange of the row-sharded table as an ALL-TO-ALL (sharded.py): rank q asks owner o only for the rows o owns.
// shard_bucket_kernel splits q's ascending unique id list by owner into W request lists of pp_cap slots (ascending, PAD
// beyond the count) and remembers where each requested id sits in the unique list (pos), so that the rows coming back can be
// put straight at their place in the compact block.  One workgroup; wave w serves owners w, w + 16, ...: a ballot
// compaction over the list keeps each bucket in list order (deterministic, no atomics).  An owner with more than pp_cap
// hits sets PXR_STATUS_SHARD_OVERFLOW (its surplus is dropped -- the host raises at the next status check).
__global__ void __launch_bounds__(1024) shard_bucket_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ n_dev,
                                                            int W, int64_t n_table, int pp_cap, int64_t pad,
                                                            int64_t* __restrict__ req, int32_t* __restrict__ pos,
                                                            int32_t* __restrict__ counts, int* status) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = *n_dev;
  for (int o = wave; o < W; o += 16) {
    int cnt = 0;
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      const int64_t id = i < n ? ids[i] : -1;
      const bool mine = id > 0 && id < n_table && (int)(id % W) == o;
      const unsigned long long m = __ballot(mine);
      if (mine) {
        const int j = cnt + __popcll(m & ((1ull << lane) - 1ull));
        if (j < pp_cap) { req[(int64_t)o * pp_cap + j] = id; pos[(int64_t)o * pp_cap + j] = i; }
      }
      cnt += __popcll(m);
    }
    for (int j = min(cnt, pp_cap) + lane; j < pp_cap; j += 64) { req[(int64_t)o * pp_cap + j] = pad; pos[(int64_t)o * pp_cap + j] = -1; }
    if (lane == 0) {
      counts[o] = cnt;
      if (cnt > pp_cap && status) atomicOr(status, PXR_STATUS_SHARD_OVERFLOW);
    }
  }
}
// dst[row_offset + pos[i], :] = src[i, :] for pos[i] >= 0: one wave per source row
__global__ void __launch_bounds__(256) scatter_rows_kernel(const float* __restrict__ src, const int32_t* __restrict__ pos,
                                                           int64_t n_src, int D, float* __restrict__ dst, int64_t dst_rows,
                                                           int row_offset) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n_src) return;
  const int64_t r = pos[i];
  if (r < 0 || r + row_offset >= dst_rows) return;
  const float4* s4 = reinterpret_cast<const float4*>(src + i * D);
  float4* d4 = reinterpret_cast<float4*>(dst + (r + row_offset) * D);
  for (int c = lane; c < D / 4; c += 64) d4[c] = s4[c];
}
}  // namespace pxr

extern "C" int pxr_shard_bucket_ids_i64(const int64_t* ids, const int32_t* n_dev, int W, int64_t n_table, int64_t pp_cap,
                                        int64_t pad_id, int64_t* req, int32_t* pos, int32_t* counts, void* stream) {
  PXR_REQUIRE(ids && n_dev && req && pos && counts, "pxr_shard_bucket_ids_i64: null pointer");
  PXR_REQUIRE(W >= 1 && W <= 1024 && n_table > 0 && pp_cap > 0 && pp_cap < (1ll << 30) && pad_id >= n_table,
              "pxr_shard_bucket_ids_i64: bad args");
  hipLaunchKernelGGL(pxr::shard_bucket_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, ids, n_dev, W, n_table, (int)pp_cap,
                     pad_id, req, pos, counts, pxr_status_word());
  return pxr_check_launch("pxr_shard_bucket_ids_i64");
}

extern "C" int pxr_scatter_rows_f32(const float* src, const int32_t* pos, int64_t n_src, int D, float* dst, int64_t dst_rows,
                                    int row_offset, void* stream) {
  PXR_REQUIRE(n_src >= 0 && D > 0 && D % 4 == 0 && dst_rows >= 0 && row_offset >= 0, "pxr_scatter_rows_f32: bad shape");
  if (n_src == 0) return PXR_OK;
  PXR_REQUIRE(src && pos && dst, "pxr_scatter_rows_f32: null pointer");
  PXR_REQUIRE((n_src + 3) / 4 < (1ll << 31), "pxr_scatter_rows_f32: too many rows");
  hipLaunchKernelGGL(pxr::scatter_rows_kernel, dim3((unsigned)((n_src + 3) / 4)), dim3(256), 0, (hipStream_t)stream, src, pos,
                     n_src, D, dst, dst_rows, row_offset);
  return pxr_check_launch("pxr_scatter_rows_f32");
}

extern "C" int pxr_shard_local_rows_i64(const int64_t* ids, int64_t n, int W, int rank, int64_t n_table,
                                        int64_t* local_rows, void* stream) {
  PXR_REQUIRE(n >= 0 && W >= 1 && rank >= 0 && rank < W && n_table > 0, "pxr_shard_local_rows_i64: bad args");
  if (n == 0) return PXR_OK;
  PXR_REQUIRE(ids && local_rows, "pxr_shard_local_rows_i64: null pointer");
  hipLaunchKernelGGL(pxr::shard_local_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     ids, n, W, rank, n_table, local_rows);
  return pxr_check_launch("pxr_shard_local_rows_i64");
}

extern "C" int pxr_ids_to_compact_i64(const int64_t* ids, int64_t n, const int64_t* uniq_idx, const int32_t* n_uniq_dev,
                                      int64_t* out, void* stream) {
  PXR_REQUIRE(n >= 0, "pxr_ids_to_compact_i64: negative n");
  if (n == 0) return PXR_OK;
  PXR_REQUIRE(ids && uniq_idx && n_uniq_dev && out, "pxr_ids_to_compact_i64: null pointer");
  hipLaunchKernelGGL(pxr::ids_to_compact_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     ids, n, uniq_idx, n_uniq_dev, out);
  return pxr_check_launch("pxr_ids_to_compact_i64");
}

extern "C" int pxr_shard_first_rows_i64(const int64_t* ids_all, int W, int64_t cap, int rank, int64_t n_table,
                                        int64_t* local_rows, void* stream) {
  PXR_REQUIRE(W >= 1 && rank >= 0 && rank < W && cap >= 0 && n_table > 0 && (int64_t)W * cap < (1ll << 31),
              "pxr_shard_first_rows_i64: bad args");
  if (cap == 0) return PXR_OK;
  PXR_REQUIRE(ids_all && local_rows, "pxr_shard_first_rows_i64: null pointer");
  const int64_t n = (int64_t)W * cap;
  hipLaunchKernelGGL(pxr::shard_first_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     ids_all, W, (int)cap, rank, n_table, local_rows);
  return pxr_check_launch("pxr_shard_first_rows_i64");
}
