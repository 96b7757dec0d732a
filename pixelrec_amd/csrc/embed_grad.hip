// embed_grad.hip -- gradient of the item-embedding table in SPARSE form (K1' of SURVEY.md §2.1).
//
// The reference's nn.Embedding (sasrec.py:31, no sparse=True) makes autograd materialise a dense [N, D] gradient
// (819 MB at N=400K, D=512: zero-fill + scatter-add, `embedding_dense_backward`) that DDP then all-reduces.
// Here the gradient is never dense: the (<= 3*B*L) row occurrences of a step are de-duplicated into
//     uniq_idx[n_uniq] (ascending item ids, id 0 = padding_idx dropped)   and   uniq_rows[n_uniq, D]
// by a stable LSD radix sort of the occurrence ids (occ_sort.cuh) followed by a segmented sum in occurrence order, so the
// result is bit-reproducible (no float atomics) and identical on every rank given identical inputs.  This file: the segment
// sums, their three sinks and the gradient entries; the rank merge of the sparse rows is merge_rows.hip.
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
#include "occ_sort.cuh"
#include "pxr_common.h"
#include "reduce_multi.cuh"

namespace pxr {

// ------------------------------------------------------------------------------------------------ segmented sum
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

}  // namespace pxr

using namespace pxr;

// Each gradient entry below reads: checks, sort_occurrences where it sorts, fill the sources, launch.

// workgroups of a segment-sum launch over n occurrences (the kernels stride over the unique rows)
static int segsum_grid(int64_t n) { return (int)(n < 4096 ? n : 4096); }
// [a, a + a_bytes) and [b, b + b_bytes) share no byte
static bool disjoint(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const char *a0 = (const char*)a, *b0 = (const char*)b;
  return a0 + a_bytes <= b0 || b0 + b_bytes <= a0;
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
  const char* who = "pxr_embed_grad_rows_f32";
  hipStream_t st = (hipStream_t)stream;
  SortWs w;
  if (int rc = carve_checked(who, ws, ws_bytes, (int)n, &w)) return rc;
  SegSumArgs a{};
  if (int rc = sort_occurrences<MODE_ROWS>(who, idx, (int)n, 0, 0, OccLayout{}, n_table, w, uniq_idx, n_uniq_dev, st, &a.vals)) return rc;
  a.seg_start = w.seg_start; a.n_uniq = n_uniq_dev; a.src0 = rows; a.uniq_rows = uniq_rows;
  a.scale = scale; a.D = D; a.T = (int)n;
  hipLaunchKernelGGL(segsum_kernel<MODE_ROWS>, dim3(segsum_grid(n)), dim3(SEG_THREADS), SEG_THREADS * 16, st, a, TailRider{});
  return pxr_check_launch(who);
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
  const char* who = "pxr_pool_table_grad_f32";
  const int n = B * (L + 2);
  hipStream_t st = (hipStream_t)stream;
  SortWs sw;
  if (int rc = carve_checked(who, ws, ws_bytes, n, &sw)) return rc;
  SegSumArgs a{};
  if (int rc = sort_occurrences<MODE_ROWS>(who, gidx, n, 0, 0, OccLayout{}, n_table, sw, uniq_idx, n_uniq_dev, st, &a.vals)) return rc;
  a.seg_start = sw.seg_start; a.n_uniq = n_uniq_dev; a.src0 = G; a.coef = w; a.uniq_rows = uniq_rows;
  a.scale = 1.f; a.D = D; a.T = B * L; a.L = L;
  hipLaunchKernelGGL(segsum_kernel<MODE_POOL>, dim3(segsum_grid(n)), dim3(SEG_THREADS), SEG_THREADS * 16, st, a, TailRider{});
  return pxr_check_launch(who);
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
  const int D = a.D;
  SortWs sw;
  if (int rc = carve_checked(who, ws, ws_bytes, n, &sw)) return rc;
  { int* t = sw.keysB; sw.keysB = sw.valsA; sw.valsA = t; }     // slots (0, 1) = pair A, (2, 3) = pair B
  int64_t* uniq_idx = (int64_t*)(final_vals_buffer(sw, n, n_rows) == sw.valsB ? sw.keysA : sw.keysB);
  int32_t* n_uniq_dev = sw.blk + sw.nblk;
  const int64_t n4 = n_rows * (D / 4);
  hipLaunchKernelGGL(dense_zero_kernel, dim3((unsigned)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096)), dim3(256), 0, st, (float4*)d_rows, n4);
  if (int rc = sort_occurrences<SORT>(who, src, n, B, L, lay, n_rows, sw, uniq_idx, n_uniq_dev, st, &a.vals)) return rc;
  a.seg_start = sw.seg_start; a.n_uniq = n_uniq_dev;
  SegStoreDense s{};
  s.d_rows = d_rows; s.uniq_idx = uniq_idx; s.n_rows = n_rows; s.D = D;
  hipLaunchKernelGGL(segsum_dense_kernel<MODE>, dim3(segsum_grid(n)), dim3(SEG_THREADS), SEG_THREADS * 16, st, a, s);
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
  PXR_REQUIRE(disjoint(d_rows, n_rows * D * 4, G, (int64_t)3 * B * D * 4), "pxr_pool_dense_grad_f32: d_rows must not alias G");
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
  PXR_REQUIRE(disjoint(d_rows, n_rows * D * 4, rows, n * D * 4), "pxr_embed_grad_dense_f32: d_rows must not alias rows");
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
  const char* who = "pxr_seq_occ_sort";
  const OccLayout lay{id_bstride, in_off, pos_off, neg_off};
  PXR_REQUIRE(occ_layout_ok(L, lay), "pxr_seq_occ_sort: bad id layout");
  PXR_REQUIRE(items && uniq_idx && n_uniq_dev && ws, "pxr_seq_occ_sort: null pointer");
  const int64_t n64 = (int64_t)3 * B * L;
  PXR_REQUIRE(B > 0 && L > 0 && n64 < (1ll << 30) && n_table > 0 && n_table < (1ll << 31), "pxr_seq_occ_sort: bad shape");
  SortWs w;
  if (int rc = carve_checked(who, ws, ws_bytes, (int)n64, &w)) return rc;
  const int* sorted_vals = nullptr;   // phase 2 finds them again: final_vals_buffer
  return sort_occurrences<MODE_SASREC>(who, items, (int)n64, B, L, lay, n_table, w, uniq_idx, n_uniq_dev, (hipStream_t)stream, &sorted_vals);
}

// pxr_seq_occ_sort + pxr_sasrec_occ_segsum(scale = 1) in one call with the DENSE sink (MOBERT4Rec: the "table" is E =
// visual_encoder(the batch's distinct images), whose gradient autograd takes dense): d_rows [n_rows, D] gets, at every referenced
// row in (0, n_rows), the row the two phases leave in uniq_rows for that id, bit for bit -- the same keys under the same layout, the
// same sort, segsum_body<MODE_SASREC>, another sink -- and exactly +0.0 everywhere else, whatever it held before (zeroed here, on the
// same stream).  Key 0 and ids outside [0, n_rows) are dropped; the latter set the bad-index bit, as in pxr_seq_occ_sort.
extern "C" int pxr_seq_occ_dense_f32(const int64_t* items, int B, int L, int64_t id_bstride, int64_t in_off, int64_t pos_off,
                                     int64_t neg_off, const float* dx0, const float* out, const float* coef, int D, int64_t n_rows,
                                     float* d_rows, void* ws, int64_t ws_bytes, void* stream) {
  const OccLayout lay{id_bstride, in_off, pos_off, neg_off};
  PXR_REQUIRE(occ_layout_ok(L, lay), "pxr_seq_occ_dense_f32: bad id layout");
  PXR_REQUIRE(items && dx0 && out && coef && d_rows && ws, "pxr_seq_occ_dense_f32: null pointer");
  const int64_t n64 = (int64_t)3 * B * L;
  PXR_REQUIRE(B > 0 && L > 0 && n64 < (1ll << 30) && D > 0 && D % 4 == 0 && D <= 4096 && n_rows > 0 && n_rows < (1ll << 31),
              "pxr_seq_occ_dense_f32: bad shape (B=%d, L=%d, D=%d)", B, L, D);
  PXR_REQUIRE((((uintptr_t)dx0 | (uintptr_t)out | (uintptr_t)d_rows) & 15) == 0,
              "pxr_seq_occ_dense_f32: dx0, out and d_rows must be 16-byte aligned");
  const int64_t src_bytes = (int64_t)B * L * D * 4;
  PXR_REQUIRE(disjoint(d_rows, n_rows * D * 4, dx0, src_bytes) && disjoint(d_rows, n_rows * D * 4, out, src_bytes),
              "pxr_seq_occ_dense_f32: d_rows must not alias dx0 or out");
  SegSumArgs a{};
  a.src0 = dx0; a.src1 = out; a.coef = coef; a.scale = 1.f; a.D = D; a.T = B * L;
  return dense_grad<MODE_SASREC, MODE_SASREC>("pxr_seq_occ_dense_f32", items, (int)n64, B, L, lay, a, n_rows, d_rows, ws, ws_bytes,
                                              (hipStream_t)stream);
}

// The MODE_SASREC argument block of phase 2 over the state pxr_seq_occ_sort left in `ws`, for entry point `who`.
// Who touches what in a phase-2 launch that carries a rider (nothing is shared, so the rider blocks need no ordering against
// the carrier's):
//   carrier: reads the occurrence workspace ws (sorted ids, segment bounds), n_uniq_dev, dx0, out, coef; writes uniq_rows -- or,
//            with the apply sink, reads uniq_idx, the hyper slot of step t_prev + 1 and the optimizer's step counter step_dev,
//            reads and writes the touched rows of table / m / v and their last[] marks, and may raise the status word;
//   rider:   reads the partial workspaces of the LayerNorm / column-sum first stages and lossrow; writes the slices of the
//            flat gradient buffer (LN gamma|beta, biases, positions), the DROPOUT step counter (another word than step_dev: no
//            segment-sum kernel reads it) and the loss scalar.
static int sasrec_phase2_args(const char* who, const void* ws, int64_t ws_bytes, int B, int L, const float* dx0, const float* out,
                              const float* coef, int D, int64_t n_table, float scale, const int32_t* n_uniq_dev, float* uniq_rows,
                              SegSumArgs* a) {
  const int n = 3 * B * L;
  SortWs w;
  if (int rc = carve_checked(who, ws, ws_bytes, n, &w)) return rc;
  *a = SegSumArgs{};
  a->vals = final_vals_buffer(w, n, n_table); a->seg_start = w.seg_start; a->n_uniq = n_uniq_dev; a->src0 = dx0; a->src1 = out;
  a->coef = coef; a->uniq_rows = uniq_rows; a->scale = scale; a->D = D; a->T = B * L;
  return PXR_OK;
}

// Phase 2: uniq_rows[u,:] = scale * sum over the occurrences of unique id u (see the header comment for the terms).
extern "C" int pxr_sasrec_occ_segsum(const void* ws, int64_t ws_bytes, int B, int L, const float* dx0, const float* out,
                                     const float* coef, int D, int64_t n_table, float scale,
                                     const int32_t* n_uniq_dev, float* uniq_rows, void* stream, const void* rider) {
  PXR_REQUIRE(ws && dx0 && out && coef && n_uniq_dev && uniq_rows, "pxr_sasrec_occ_segsum: null pointer");
  PXR_REQUIRE(B > 0 && L > 0 && D > 0 && D % 4 == 0, "pxr_sasrec_occ_segsum: bad shape");
  const char* who = "pxr_sasrec_occ_segsum";
  SegSumArgs a;
  if (int rc = sasrec_phase2_args(who, ws, ws_bytes, B, L, dx0, out, coef, D, n_table, scale, n_uniq_dev, uniq_rows, &a)) return rc;
  TailRider r;
  if (int rc = pxr_tail_rider_prepare(rider, who, &r)) return rc;
  hipLaunchKernelGGL(segsum_kernel<MODE_SASREC>, dim3(segsum_grid(3 * B * L) + r.blocks), dim3(SEG_THREADS), SEG_THREADS * 16,
                     (hipStream_t)stream, a, r);
  return pxr_check_launch(who);
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
  const char* who = "pxr_sasrec_occ_segsum_apply";
  SegSumArgs a;
  if (int rc = sasrec_phase2_args(who, ws, ws_bytes, B, L, dx0, out, coef, D, n_table, 1.f, n_uniq_dev, nullptr, &a)) return rc;
  SegApplyRows s{};
  s.p = table; s.m = m; s.v = v; s.last = last; s.uniq_idx = uniq_idx; s.n_table = table_rows;
  s.hyper = (const float4*)hyper; s.step_dev = step_dev; s.t_prev = (int)t_prev; s.D = D;
  s.c = AdamConsts{(float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps};
  s.status = pxr_status_word();
  TailRider r;
  if (int rc = pxr_tail_rider_prepare(rider, who, &r)) return rc;
  hipLaunchKernelGGL(segsum_apply_kernel, dim3(segsum_grid(3 * B * L) + r.blocks), dim3(SEG_THREADS), SEG_THREADS * 16,
                     (hipStream_t)stream, a, s, r);
  return pxr_check_launch(who);
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
  SegSumArgs a;
  if (int rc = sasrec_phase2_args("pxr_sasrec_occ_segsum_split", ws, ws_bytes, B, L, dx0, out, coef, D, n_table, scale, n_uniq_dev,
                                  uniq_rows, &a)) return rc;
  int64_t o1, o2, tot;
  split_layout(n, D, &a.big_cap, &a.max_parts, &o1, &o2, &tot);
  a.split = SEG_SPLIT;
  a.big_count = (int*)ws2; a.big_rows = (int*)((char*)ws2 + o1); a.partials = (float*)((char*)ws2 + o2);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(segsum_kernel<MODE_SASREC>, dim3(segsum_grid(n)), dim3(SEG_THREADS), SEG_THREADS * 16, st, a, TailRider{});
  hipLaunchKernelGGL(segsum_parts_kernel<MODE_SASREC>, dim3(a.max_parts < 1024 ? a.max_parts : 1024), dim3(SEG_THREADS), SEG_THREADS * 16, st, a);
  hipLaunchKernelGGL(segsum_big_kernel, dim3(a.big_cap < 64 ? a.big_cap : 64), dim3(SEG_THREADS), 0, st, a);
  return pxr_check_launch("pxr_sasrec_occ_segsum_split");
}
