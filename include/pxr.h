/* pxr.h -- C ABI of libpxr.so: hand-written gfx950 (MI355X / CDNA4) HIP kernels for the PixelRec
 * sequential-recommender hot path (SASRec under IDNet).
 *
 * The reference (westlake-repl/PixelRec) is 100 % Python on stock PyTorch ops and has NO FFI of its own
 * (SURVEY.md §8b): the seam is the Python model-class contract.  These entry points are what a binding for this
 * path would bind -- plain pointers and sizes, no torch types -- and each one names the reference call site it
 * replaces (paths relative to /root/reference/code/REC/).  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - all tensors are dense row-major fp32 unless stated; indices are int64 (torch.long) like the reference's;
 *   - every pointer is a DEVICE pointer; the library never allocates, frees or retains device memory;
 *   - `stream` is a hipStream_t; calls are asynchronous, re-entrant, and hold no global mutable state
 *     (usable from the autograd thread); all launches are hipGraph-capturable (no host syncs);
 *   - return 0 on success, <0 on error (PXR_ERR_*); pxr_last_error() gives the thread-local message;
 *   - `*_ws_bytes` functions return the scratch size the matching call needs.
 *   - dropout: Bernoulli(1-p) keep-mask = counter hash of (seed, stream_id, element index); the backward call
 *     must pass the same (p, seed, stream_id).  p = 0 disables it (eval).
 *   - `step_dev` (const int64_t*, may be NULL): a device-resident step counter.  Dropout entry points add it to
 *     `seed`; optimizer entry points take the step number from it.  With it a whole training step can be captured
 *     in a hipGraph and replayed: pxr_counter_add_i64 advances the counter on the device, no host value is baked in.
 */
#ifndef PXR_H_
#define PXR_H_
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PXR_OK 0
#define PXR_ERR_BAD_ARG (-1)
#define PXR_ERR_LAUNCH (-2)
#define PXR_ERR_WORKSPACE (-3)

/* The ABI revision this header describes.  pxr_version() of the loaded library must EQUAL it: entries may change meaning between
 * revisions while keeping their names (0.2.0 -> 0.3.0: the `stat` buffers of pxr_ln_bwd_stat_f32 / pxr_attn_bwd_stat_f32 became
 * pxr_ln_bwd_partial_rows(rows) / 64 words instead of one caller-zeroed word, and pxr_ln_bwd_stat_f32 gained `zero`, `zero_n`),
 * so a caller built against another revision must refuse to run instead of writing out of bounds (pixelrec_amd/lib.py does).
 * 0.3.0 -> 0.3.1: one entry per kernel family -- the plane-writing, h2, bidirectional and id-layout variants were folded into the
 * plain names, which now take the most general argument list (planes triple + planes_fmt, causal, id layout); the shims died. */
#define PXR_ABI_VERSION 302
int pxr_version(void);                 /* major*10000 + minor*100 + patch; == PXR_ABI_VERSION of the header it was built from */
const char* pxr_last_error(void);      /* message of the last failing call on this thread */
const char* pxr_target_arch(void);     /* "gfx950" */

/* HOST function: keep-mask bytes (1 = keep) of elements first_index .. first_index+n-1 for (seed, stream_id, p),
 * computed with the same hash the kernels use.  For tests of the dropout restatement; no device work. */
int pxr_dropout_keep_host(uint64_t seed, uint32_t stream_id, uint64_t first_index, int64_t n, float p,
                          uint8_t* keep_out);

/* Registers a caller-owned int32 in DEVICE memory as this process' status word (NULL unregisters).  Kernels that
 * gather table rows by id (pxr_embed_gather_f32, pxr_input_ln_fwd_f32, the loss head's target / negative ids in
 * pxr_bpr_loss_fwd_f32 and pxr_ln_residual_bpr_fwd_f32, the occurrence ids of pxr_seq_occ_sort) OR bit 0 into it when an id lies
 * outside [0, N) -- where the reference's nn.Embedding raises IndexError / a device-side assert (model/IDNet/sasrec.py:68) --
 * and clamp (the sort: drop) the id; pxr_merge_split_rows_f32 ORs bit 1 when a rank's row count exceeded the exchanged capacity.  The
 * host reads the word at its next synchronisation point and raises.  One process per GPU. */
int pxr_set_status_word(int32_t* dev_word);

/* ---- embedding table ---------------------------------------------------------------------------------------- */
/* out[i,:] = table[idx[i],:]                       model/IDNet/sasrec.py:68,101; model/PixelNet/mosasrec.py:102 */
int pxr_embed_gather_f32(const float* table, int64_t N, int D, const int64_t* idx, int64_t n, float* out,
                         void* stream);

/* Sparse embedding backward (replaces autograd's dense embedding_dense_backward of sasrec.py:31/68):
 * (idx[n], rows[n,D]) -> ascending uniq_idx[<=n], uniq_rows[<=n,D] = scale * sum of the rows of each id,
 * *n_uniq_dev = count.  Id 0 (padding_idx) and out-of-range ids are dropped.  Deterministic (stable sort).
 * csrc/embed_grad.hip (the segment sums and every table-gradient entry) on the occurrence sort of csrc/occ_sort.cuh. */
int64_t pxr_embed_grad_ws_bytes(int64_t n_occ);
int pxr_embed_grad_rows_f32(const int64_t* idx, int64_t n, const float* rows, int D, int64_t n_table, float scale,
                            int64_t* uniq_idx, float* uniq_rows, int32_t* n_uniq_dev, void* ws, int64_t ws_bytes,
                            void* stream);
/* Data-parallel merge of the W rank-local sparse gradients after the all-gather (the build's replacement of DDP's
 * dense all-reduce, run.py:40): idx_all[W,cap] / rows_all[W,cap,D], every list ascending and unique over its whole
 * cap (unused tail slots hold ids >= n_table).  No re-sort: the lowest rank holding an id owns it and adds the other
 * ranks' rows in rank order (same fixed order on every replica).  Output is not compacted: out_idx[e] = id or 0
 * (empty slot, skipped by pxr_adamw_rows_f32 / pxr_adamw_table_f32), out_rows[e,:] = scale * sum, *n_out = W*cap.
 * csrc/merge_rows.hip. */
int64_t pxr_merge_rows_ws_bytes(int W, int64_t cap);
int pxr_merge_sorted_rows_f32(const int64_t* idx_all, const float* rows_all, int W, int64_t cap, int D,
                              int64_t n_table, float scale, int64_t* out_idx, float* out_rows, int32_t* n_out_dev,
                              void* ws, int64_t ws_bytes, void* stream);
/* The same merge on the layout a ONE-collective exchange delivers: packed_all = W blocks of pxr_packed_rows_bytes(cap, D)
 * bytes, block = { int64 ids[cap] ascending over the first `count` entries; int32 count; zero padding to a 16-byte
 * boundary (rows start at pxr_packed_rows_offset(cap)); float rows[cap][D] }.  Entries at or beyond a block's count
 * are ignored whatever they hold, so a rank sends its sort/segment output as it is (no PAD fill, no second
 * all-gather for the ids).  Same output convention, same summation order as pxr_merge_sorted_rows_f32. */
int64_t pxr_packed_rows_offset(int64_t cap);
int64_t pxr_packed_rows_bytes(int64_t cap, int D);
int pxr_merge_packed_rows_f32(const void* packed_all, int W, int64_t cap, int D, int64_t n_table, float scale,
                              int64_t* out_idx, float* out_rows, int32_t* n_out_dev, void* ws, int64_t ws_bytes,
                              void* stream);
/* The exchange with a REDUCED row capacity cap_x <= cap (two collectives): heads_all = W x pxr_packed_rows_offset(cap)
 * bytes ({ids[cap], count, pad} of every rank), rows_all = [W, cap_x, D] (the first cap_x rows of every rank).  A rank
 * whose count exceeds cap_x is cut there and bit 1 of the status word (pxr_set_status_word) is set.  out_*: W*cap_x slots. */
int pxr_merge_split_rows_f32(const void* heads_all, const float* rows_all, int W, int64_t cap, int64_t cap_x, int D,
                             int64_t n_table, float scale, int64_t* out_idx, float* out_rows, int32_t* n_out_dev,
                             void* ws, int64_t ws_bytes, void* stream);
/* On-device train-batch construction (data/dataset/trainset.py:40-63): pos int64 [B,W] left-padded windows (W = L+1)
 * -> items [B,2,W] (positives | one negative per target position, uniform over [1, n_items-1] minus the window's own
 * items) and masked_index [B,W-1].  Stateless: (seed, batch_counter) select the random stream. */
int pxr_sample_negatives_i64(const int64_t* pos, int B, int W, int64_t n_items, uint64_t seed, uint64_t batch_counter,
                             int64_t* items, int64_t* masked_index, void* stream);

/* Row-sharded table, hit-row exchange as an all-to-all (model/sharded.py): split a rank's ascending unique id list (count on
 * the device) by owner (id % W) into W request lists of pp_cap slots -- req[W, pp_cap] ascending, pad_id beyond the count;
 * pos[W, pp_cap] = the id's index in the unique list (-1 for padding); counts[W].  An owner with more than pp_cap hits sets
 * status bit 16 (PXR_STATUS_SHARD_OVERFLOW) and loses its surplus.  pxr_scatter_rows_f32: dst[row_offset + pos[i], :] =
 * src[i, :] for pos[i] >= 0 (the rows that came back, put at their place in the compact block). */
int pxr_shard_bucket_ids_i64(const int64_t* ids, const int32_t* n_dev, int W, int64_t n_table, int64_t pp_cap, int64_t pad_id,
                             int64_t* req, int32_t* pos, int32_t* counts, void* stream);
int pxr_scatter_rows_f32(const float* src, const int32_t* pos, int64_t n_src, int D, float* dst, int64_t dst_rows,
                         int row_offset, void* stream);
/* Row-sharded table (csrc/shard.hip; north_star "embedding table optionally row-sharded", BASELINE configs[3]): owner of id =
 * id % W, its row in the owner's shard = id / W + 1 (local row 0 = all-zero dummy).  local_rows[i] = that row if this
 * rank owns ids[i] (0 < id < n_table), else 0.  pxr_ids_to_compact: out[i] = 1 + position of ids[i] in the ascending
 * unique list (0 for padding): re-indexes a batch onto the [n_uniq+1, D] block of rows fetched from the owners. */
int pxr_shard_local_rows_i64(const int64_t* ids, int64_t n, int W, int rank, int64_t n_table, int64_t* local_rows,
                             void* stream);
int pxr_ids_to_compact_i64(const int64_t* ids, int64_t n, const int64_t* uniq_idx, const int32_t* n_uniq_dev,
                           int64_t* out, void* stream);
/* ids_all[W,cap]: W ascending request lists (tail >= n_table).  Like pxr_shard_local_rows_i64, but an id requested by
 * several ranks keeps its local row only in the lowest-ranked list: the duplicate-free work list of the owner's lazy
 * AdamW catch-up. */
int pxr_shard_first_rows_i64(const int64_t* ids_all, int W, int64_t cap, int rank, int64_t n_table,
                             int64_t* local_rows, void* stream);
/* The table gradient of the three uses of the table inside SASRec.forward (sasrec.py:68-74,88-89) without materialising the
 * [B,2,L+1,D] gather, in two phases: phase 1 depends on `items` only and may run before the forward pass (the lazy table
 * optimizer brings exactly these unique rows up to date before they are read); `ws` (pxr_embed_grad_ws_bytes(3*B*L) bytes)
 * carries the sorted occurrences to phase 2 and must not be touched in between.  Phase 1: the input ids at in_off, targets at
 * pos_off, negatives at neg_off of each sequence's id_bstride ids -- SASRec's items [B,2,L+1]: (2(L+1), 0, 1, L+2); BERT4Rec's
 * [B,3,L]: (3L, 0, L, 2L), the table's three uses in bert4rec.py:76-81 under autograd.  Phase 2: dx0 = grad of (table row + pos)
 * [B*L,D]; out = last-layer states [B*L,D]; coef[B*L] from pxr_bpr_loss_bwd_f32, whatever the layout.  Deterministic, no float
 * atomics, row 0 dropped, every other row (BERT4Rec's mask token item_num included) ordinary. */
int pxr_seq_occ_sort(const int64_t* items, int B, int L, int64_t id_bstride, int64_t in_off, int64_t pos_off, int64_t neg_off,
                     int64_t n_table, int64_t* uniq_idx, int32_t* n_uniq_dev, void* ws, int64_t ws_bytes, void* stream);
/* A TAIL RIDER: small reductions that close a backward pass and share no byte with the segment sums, run by extra workgroups
 * appended to the grid of the ONE phase-2 launch instead of by launches of their own.  n (0..16) partial-reduction problems with
 * the meaning of pxr_reduce_partials_multi_f32's arguments (out_b[i] NULL: single output; bump_counter optional), and, when
 * loss != NULL, the loss sum loss[0] = (1/B) sum_b sum_t lossrow[b*L + t] that pxr_ln_residual_bpr_fwd_f32(loss = NULL) left
 * undone.  Same code, same association, same bits as the stand-alone launches.  The descriptor is host memory, read during the
 * call only.  The caller guarantees that none of its buffers is one the carrier reads or writes. */
typedef struct pxr_tail_rider {
  int32_t n, B, L, reserved;
  const float* part[16];
  float* out_a[16];
  float* out_b[16];
  int32_t P[16], N[16], split[16];
  int64_t* bump_counter;
  const float* lossrow;
  float* loss;
} pxr_tail_rider;
/* rider: a pxr_tail_rider or NULL (none) */
int pxr_sasrec_occ_segsum(const void* ws, int64_t ws_bytes, int B, int L, const float* dx0, const float* out,
                          const float* coef, int D, int64_t n_table, float scale, const int32_t* n_uniq_dev,
                          float* uniq_rows, void* stream, const void* rider);
/* Phase 2 with the lazy AdamW row update inside (one rank, lazy table update, scale 1): one launch leaves in table / m / v / last
 * what pxr_sasrec_occ_segsum followed by pxr_adamw_rows_f32(rows = uniq_idx, grows = uniq_rows, t_apply = t_prev + 1) leaves there
 * for rows that are current through t_prev, bit for bit; the summed rows are applied where they are formed and never written.
 * uniq_idx / n_uniq_dev: phase 1's output.  hyper: the per-step scalars (pxr_adamw_hyper_append; entry t_prev + 1 must exist);
 * step_dev != NULL: t_prev = *step_dev.  A row with last[row] != t_prev is left untouched and raises status bit 256
 * (PXR_STATUS_ROWS_STALE); id 0 and ids outside [0, table_rows) are skipped.  Every segment is summed by one workgroup: batches
 * that want pxr_sasrec_occ_segsum_split keep the two launches.  rider: a pxr_tail_rider or NULL (none). */
int pxr_sasrec_occ_segsum_apply(const void* ws, int64_t ws_bytes, int B, int L, const float* dx0, const float* out,
                                const float* coef, int D, int64_t n_table, const int32_t* n_uniq_dev, const int64_t* uniq_idx,
                                float* table, float* m, float* v, int32_t* last, int64_t table_rows, const void* hyper,
                                int64_t t_prev, const int64_t* step_dev, double beta1, double beta2, double eps, void* stream,
                                const void* rider);

/* Phase 2 for big batches (round 5): the same sums, with the rows of more than 1 024 occurrences (a Zipf-popular item of a
 * 2 048-sequence batch has 13 000) cut into parts of 512 occurrences that many workgroups sum, the parts of a row added in part
 * order -- three launches instead of one, worth it from ~30 000 occurrences.  Bit-reproducible; long rows are associated
 * differently from pxr_sasrec_occ_segsum (part by part).  ws2: pxr_sasrec_occ_split_ws_bytes(B, L, D) bytes (0 = shape not
 * served) whose first 256 bytes are ZERO at the first call; every call leaves them zero.  Replaces the scatter-add of the
 * embedding backward (sasrec.py:68 autograd), as pxr_sasrec_occ_segsum does. */
int64_t pxr_sasrec_occ_split_ws_bytes(int B, int L, int D);
int pxr_sasrec_occ_segsum_split(const void* ws, int64_t ws_bytes, int B, int L, const float* dx0, const float* out,
                                const float* coef, int D, int64_t n_table, float scale, const int32_t* n_uniq_dev,
                                float* uniq_rows, void* ws2, int64_t ws2_bytes, void* stream);

/* ---- LayerNorm sites ---------------------------------------------------------------------------------------- */
/* y = dropout(LN(table[idx[b*idx_bstride+t]] + pos[t]))       sasrec.py:68,77-82 (train) / :99-104 (predict).
 * xhat [B*L,D] / rstd [B*L] are saved for the backward and may be NULL for inference.  y is ALSO written as planes (see
 * "pre-split operands" below; y_planes NULL: none) in the format planes_fmt: 0 = bf16x3, 1 = h2 (y_planes then required). */
int pxr_input_ln_fwd_f32(const float* table, int64_t n_table, const int64_t* idx, int64_t idx_bstride,
                         const float* pos, const float* gamma, const float* beta, float eps, int B, int L, int D,
                         float* y, float* xhat, float* rstd, float p_drop, uint64_t seed, uint32_t stream_id,
                         const int64_t* step_dev, void* y_planes, int64_t y_plane_stride, int64_t y_panel_rows, int planes_fmt,
                         void* stream);
/* y = LN(dropout(x) + res)                                      layers.py:614-615 and :670-671
 * y as planes as above; y may then be NULL (h2: y_planes required). */
int pxr_ln_residual_fwd_f32(const float* x, const float* res, const float* gamma, const float* beta, float eps,
                            int rows, int D, float* y, float* xhat, float* rstd, float p_drop, uint64_t seed,
                            uint32_t stream_id, const int64_t* step_dev, void* y_planes, int64_t y_plane_stride,
                            int64_t y_panel_rows, int planes_fmt, void* stream);
/* The residual site reading its rows from a per-item cache: x_out[i,t,:] = cache[ids[i]*T + t, :] and y = LN(x_out), rows = n*T.
 * The reference encodes every image of a step through the whole tower (model/PixelNet/mosasrec.py:69) and every item again per
 * evaluation (trainer/trainer.py:339-355), although the first `tune_scale` parameters are frozen (model/load.py:97-99): with no
 * dropout in CLIP and no augmentation in the store, the activation entering the first trainable block is a function of the item
 * id alone.  cache [n_items, T*D] holds it per item; this entry is the first launch of that block -- its gather and its first
 * LayerNorm in one pass.  x_out (required) is the block's residual input; y fp32 and / or planes (planes_fmt as above, unit
 * scale), xhat [n*T,D] / rstd [n*T] optional: pxr_ln_residual_fwd_f32's outputs without dropout and `res`, and the same bits as
 * pxr_embed_gather_f32 on the [n_items, T*D] view followed by it.  Offsets are 64-bit (the cache may exceed 2^31 elements; n*T
 * may not); an id outside [0, n_items) sets PXR_STATUS_BAD_INDEX and is clamped. */
int pxr_ln_gather_fwd_f32(const float* cache, int64_t n_items, const int64_t* ids, int n, int T, const float* gamma,
                          const float* beta, float eps, int D, float* x_out, float* y, float* xhat, float* rstd,
                          void* y_planes, int64_t y_plane_stride, int64_t y_panel_rows, int planes_fmt, void* stream);
/* autograd of either site.  gather_mode=1: dy is w.r.t. the dropped output, dz = grad of (table row + pos).
 * gather_mode=0: dz = grad w.r.t. res, dx (optional) = grad w.r.t. x.  dgamma/dbeta are overwritten; pass both NULL to
 * defer the final reduction (partials stay in ws, reduce them with pxr_reduce_partials_multi_f32).  g_planes (residual sites
 * only; NULL: none): the gradient the next GEMMs read (dx when given, else dz) also as bf16x3 planes. */
int64_t pxr_ln_bwd_ws_bytes(int rows, int D);
int pxr_ln_bwd_partial_rows(int rows);   /* rows of the [P, 2*D] partial buffer left in ws when dgamma/dbeta are NULL */
int pxr_ln_bwd_f32(int gather_mode, const float* dy, const float* xhat, const float* rstd, const float* gamma,
                   int rows, int D, float* dz, float* dx, float* dgamma, float* dbeta, float p_drop, uint64_t seed,
                   uint32_t stream_id, const int64_t* step_dev, void* ws, int64_t ws_bytes, void* g_planes,
                   int64_t g_plane_stride, int64_t g_panel_rows, void* stream);

/* ---- fp32 MFMA GEMMs (v_mfma_f32_32x32x2_f32) --------------------------------------------------------------- */
/* General: C[M,N] = A_op x B_op; a_kc/b_kc select k-contiguous ([M][K] / [N][K]) or x-contiguous ([K][M] / [K][N])
 * storage.  epilogue: 0 none, 1 +bias[n], 2 +bias then erf-GELU (pre-activation -> aux), 3 *= gelu'(aux), 4 += aux,
 * 5 +bias then erf-GELU (gelu'(pre-activation) -> aux), 6 *= aux. */
int64_t pxr_gemm_ws_bytes(int a_kc, int b_kc, int M, int N, int K);
int pxr_gemm_f32(int a_kc, int b_kc, int M, int N, int K, const float* A, int64_t lda, const float* B, int64_t ldb,
                 float* C, int64_t ldc, int epilogue, const float* bias, float* aux, int64_t ldaux, void* ws,
                 int64_t ws_bytes, int tile_hint, int split_hint, void* stream);
/* `batch` independent GEMMs of one shape in one launch (grid.z).  Operand z starts (z / nb2) * x1 + (z % nb2) * x2
 * floats after its base pointer (two-level strides: image n and head h of a packed [n, T, 3*heads*d] projection).  No
 * epilogue, no split-K.  The attention contractions of the ViT image encoder (HF CLIPAttention, built by the
 * reference at model/load.py:94): S = Q K^T, O = P V, dV = P^T dO, dP = dO V^T, dQ = dS K, dK = dS^T Q. */
int pxr_gemm_batched_f32(int a_kc, int b_kc, int M, int N, int K, const float* A, int64_t lda, const float* B,
                         int64_t ldb, float* C, int64_t ldc, int batch, int nb2, int64_t a1, int64_t a2, int64_t b1,
                         int64_t b2, int64_t c1, int64_t c2, int tile_hint, void* stream);

/* GEMM mode of the process (also PXR_GEMM_MODE=bf16x3|f32, default bf16x3): with bf16x3 every product pxr_gemm_f32 /
 * pxr_gemm_batched_f32 / pxr_linear_* / pxr_grouped_linear_bwd_weight_f32 would run with its heuristic tile is computed
 * on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16) after an EXACT split of each fp32 operand into three bf16 terms,
 * six cross products, fp32 accumulation (csrc/gemm_b3.cuh: error bound ~2^-25 |a||b| per product, i.e. fp32-class;
 * tests/test_gpu_gemm_b3.py).  f32 = the f32-input MFMA kernels (v_mfma_f32_32x32x2_f32).  An explicit f32 tile_hint
 * always takes the f32 kernels; tile_hint 9064 / 91281 force the bf16x3 64x64 / 128x128 tile. */
int pxr_set_gemm_mode(int bf16x3);
int pxr_get_gemm_mode(void);

/* ---- pre-split operands ("planes"): the same fp32 products on the bf16 matrix pipe, operands split ONCE ---------- */
/* An fp32 matrix X[rows, cols] (cols % 32 == 0) as three bf16 planes hi | mid | lo with X = hi + mid + lo exactly
 * (hi = bf16(X), mid = bf16(X - hi), lo = X - hi - mid).  Plane q starts q * plane_stride ELEMENTS after `planes`; inside
 * a plane the matrix is stored as cols / 32 PANELS of panel_rows (>= rows, multiple of 32; rows past `rows` must be ZERO when the rows are a GEMM's reduction dimension) rows x 32 columns:
 *     element (r, c) at ((c / 32) * panel_rows + r) * 32 + ((((c / 8) % 4) ^ ((r / 4) % 4)) * 8 + c % 8
 * (64-byte row segments, 16-byte chunks XOR-swizzled by the row: a GEMM tile is a byte copy of 1 KiB runs, csrc/gemm_p3.cuh).
 * A row range [r0, r1) with r0 % 16 == 0 is the same layout at planes + 32 r0; a column range with c0 % 32 == 0 at
 * planes + (c0 / 32) * panel_rows * 32.  pxr_split_planes_f32 writes the planes of an operand whose producer does not
 * (weights after an optimizer step, the item table before a full-sort evaluation -- model/IDNet/sasrec.py:112,115-117). */
int pxr_split_planes_f32(const float* x, int64_t rows, int64_t cols, int64_t ldx, void* planes, int64_t plane_stride,
                         int64_t panel_rows, void* stream);
/* C[M,N] = A[M,K] x B (+ epilogue as pxr_gemm_f32) with both operands given as planes: b_kc = 1: B is [N][K] (nn.Linear
 * forward model/layers.py:586-588,613,666,669; scoring model/IDNet/sasrec.py:112), b_kc = 0: B is [K][N] (the input
 * gradient dX = dY W of the same layers).  What pxr_gemm_f32 computes in mode bf16x3, bit for bit.  K % 32 == 0.
 * C may be NULL when only the output planes (c_planes: panel layout of C, N % 32 == 0) are wanted; c_planes may be NULL. */
int pxr_gemm_planes_f32(int b_kc, int M, int N, int K, const void* A, int64_t a_plane_stride, int64_t a_panel_rows,
                        const void* B, int64_t b_plane_stride, int64_t b_panel_rows, float* C, int64_t ldc, int epilogue,
                        const float* bias, float* aux, int64_t ldaux, void* c_planes, int64_t c_plane_stride,
                        int64_t c_panel_rows, int act, int tile_hint, void* stream);

/* up to 16 matrices in one launch (host arrays of n entries): the weight matrices of the block after an optimizer step */
int pxr_split_planes_multi_f32(int n, const float* const* x, const int64_t* rows, const int64_t* cols, const int64_t* ldx,
                               void* const* planes, const int64_t* plane_stride, const int64_t* panel_rows, void* stream);
/* ---- the TWO-plane fp16 operand format ("h2", csrc/planes.cuh): x 2^e = hi + lo, both fp16, 22 significant bits; a product
 * needs three MFMAs (v_mfma_f32_32x32x16_f16) instead of the six of the 3 x bf16 split -- same accuracy, half the matrix-pipe
 * work (profiles/r04/lab/h2_lab_run1.log).  fp16 has a finite range: the producer of an operand picks the power of two 2^e
 * (exact) that places its values in it and the GEMM undoes it; a value that still leaves the range sets bit 64 of the status
 * word (pxr_set_status_word) instead of silently becoming inf.  Same panel layout as the bf16 planes, planes 0 and 1.
 * Used by the forward-only blocks of the image tower (reference: the frozen CLIP blocks of code/REC/model/load.py:90-120).
 *   pxr_split_h2_multi_f32   up to 16 matrices, matrix i multiplied by 2^scale_exp[i] first
 *   pxr_gemm_h2_f32          C = epilogue(2^-(a_exp+b_exp) A~ B~), B~ [N][K] (b_kc = 1: forward) or [K][N] (b_kc = 0: input gradient), with
 *                            the epilogues pxr_gemm_planes_f32 takes for that flavour (one list for both: csrc/gemm_epi.cuh);
 *                            exponents immediate or read from *_exp_dev; c_fmt 0: output planes as three bf16 planes, 1: as two
 *                            fp16 planes holding C 2^(*c_exp_dev) (unit scale when null)
 *   pxr_ln_residual_fwd_f32 / pxr_input_ln_fwd_f32 / pxr_attn_fwd_f32 / pxr_tower_attn_fwd_f32 with planes_fmt 1: the
 *                            plane-writing producers with h2 planes, unit scale */
int pxr_split_h2_multi_f32(int n, const float* const* x, const int64_t* rows, const int64_t* cols, const int64_t* ldx,
                           void* const* planes, const int64_t* plane_stride, const int64_t* panel_rows, const int* scale_exp,
                           void* stream);
int pxr_gemm_h2_f32(int b_kc, int M, int N, int K, const void* A, int64_t a_plane_stride, int64_t a_panel_rows, int a_exp,
                    const int* a_exp_dev, const void* B, int64_t b_plane_stride, int64_t b_panel_rows, int b_exp,
                    const int* b_exp_dev, float* C, int64_t ldc, int epilogue, const float* bias, float* aux, int64_t ldaux,
                    void* c_planes, int64_t c_plane_stride, int64_t c_panel_rows, int c_fmt, const int* c_exp_dev, int act,
                    int tile_hint, void* stream);
/* the weight gradients of pxr_grouped_dw_planes_f32 from h2 operands (exponents per problem: immediate, or read from *_exp_dev[i]) */
int pxr_grouped_dw_h2_f32(int n, const void* const* dy, const int64_t* dy_plane_stride, const int64_t* dy_panel_rows,
                          const int* dy_exp, const int* const* dy_exp_dev, const void* const* x, const int64_t* x_plane_stride,
                          const int64_t* x_panel_rows, const int* x_exp, const int* const* x_exp_dev, float* const* dW,
                          float* const* db, const int* T, const int* N, const int* K, int tile_hint, void* stream);
/* h2 split with the scale chosen ON THE DEVICE (tensors that change every step): per matrix max |x| -> stats[2 i] (col_stats: also
 * the largest column sum of |x| -> stats[2 i + 1]; col_stats 0: rows * max instead, an upper bound; col_stats 2: stats[2 i] was
 * gathered by the producers, no statistics pass) and e = top - ceil(log2 max) -> exps[i], top = 14 unless bits 8-15 of
 * col_stats name another (8 .. 15: more headroom for tensors someone rewrites in place with the same exponent -- the weight
 * planes pxr_adamw_flat_tab_ex_f32 keeps current); no host synchronisation.
 * pxr_h2_bound_exp: *exp_out = 15 - ceil(log2(a_max[0] * b_colsum[0] * factor)) -- the exponent of an input gradient that leaves
 * a GEMM epilogue as planes before its maximum can be known (|dy W| <= max |dy| * max column sum of |W|). */
int pxr_h2_split_auto_multi_f32(int n, const float* const* x, const int64_t* rows, const int64_t* cols, const int64_t* ldx,
                                void* const* planes, const int64_t* plane_stride, const int64_t* panel_rows, int col_stats,
                                float* stats, int* exps, void* stream);
int pxr_h2_bound_exp(const float* a_max, const float* b_colsum, float factor, int* exp_out, void* stream);
/* Producers that gather the statistics themselves (col_stats = 2 of pxr_h2_split_auto_multi_f32 then skips its own pass): the
 * LayerNorm backward of a residual site / the fused attention backward, as pxr_ln_bwd_f32(gather_mode 0) / pxr_attn_bwd_f32, plus
 * PARTIAL maxima of |gradient the next GEMMs read| (dx when given, else dz) / of max(|dq|, |dk|, |dv|), reduced by
 * pxr_h2_split_parts_f32: the LayerNorm backward writes stat[w] for each of its pxr_ln_bwd_partial_rows(rows) workgroups (plain
 * stores, nothing to zero) and clears `zero_n` (<= 256) floats at `zero` on request; the attention backward raises
 * PXR_ATTN_STAT_SLOTS = 64 words the caller (or that LayerNorm launch) zeroed, one atomic per workgroup.  (Round 4 raised one
 * word once per wave: thousands of same-address atomics per launch.) */
int pxr_ln_bwd_stat_f32(const float* dy, const float* xhat, const float* rstd, const float* gamma, int rows, int D, float* dz,
                        float* dx, float* dgamma, float* dbeta, float p_drop, uint64_t seed, uint32_t stream_id,
                        const int64_t* step_dev, void* ws, int64_t ws_bytes, float* stat, float* zero, int zero_n, void* stream);
/* The same site in a PRE-LN block (the image tower; HF CLIPEncoderLayer, reached from the reference's REC/model/load.py:90-120):
 * dz = res + LayerNorm-backward(dy), one launch instead of pxr_ln_bwd_f32 + pxr_add_f32 (the same bits); no dropout at these sites.
 * stat optional (NULL: no statistics). */
int pxr_ln_bwd_res_f32(const float* dy, const float* xhat, const float* rstd, const float* gamma, const float* res, int rows, int D,
                       float* dz, float* dgamma, float* dbeta, void* ws, int64_t ws_bytes, float* stat, void* stream);
int pxr_h2_split_parts_f32(const float* x, int64_t rows, int64_t cols, int64_t ldx, void* planes, int64_t plane_stride,
                           int64_t panel_rows, const float* parts, int n_parts, float* stats, int* exps,
                           const float* bound_b_colsum, float bound_factor, int* bound_exp_out, void* stream);
/* (bound_exp_out, optional: the launch also leaves the exponent pxr_h2_bound_exp would compute for the input gradient the next
 * GEMM forms from x and the weight whose column-sum statistic is *bound_b_colsum -- one one-thread launch less per use) */
int pxr_attn_bwd_stat_f32(const float* dctx, int64_t ld_ctx, const float* q, const float* k, const float* v, int64_t ld,
                          const float* probs, int B, int H, int L, int d, float* dq, float* dk, float* dv, int64_t ld_d,
                          float p_drop, uint64_t seed, uint32_t stream_id, const int64_t* step_dev, float* stat, void* stream);
/* ---- stale scales (round 6): the three h2 split launches per layer of a training step's backward pass removed.  The gradients a
 * backward pass hands to its GEMMs change slowly from step to step, so their producers write the planes THEMSELVES under an exponent
 * that exists before they run -- derived from the PREVIOUS step's maximum, `headroom` binades below the usual placement -- and leave
 * this step's partial maxima for the next derivation.  A value that outgrows the headroom is SATURATED to +-65504 (never inf) and
 * raises PXR_STATUS_H2_STALE (128) in the status word.
 * pxr_ln_bwd_h2s_f32: a residual LayerNorm site's backward (reference layers.py:614-615 / :670-671 under autograd); dz as fp32, the
 *   gradient the next GEMMs read (dropout applied when p_drop > 0; no fp32 copy) ONLY as two fp16 planes of gradient * 2^g_exp_dev[0];
 *   stat[pxr_ln_bwd_partial_rows(rows)] partial maxima; zero / zero_n as pxr_ln_bwd_stat_f32.  pos_score != NULL: the loss head's
 *   backward fused in as in pxr_bpr_ln_bwd_f32, with its id layout (dy unused, rows == B * L); NULL: the eleven head arguments
 *   are ignored (the id layout is still checked).
 * pxr_attn_bwd_h2s_f32: dq | dk | dv ONLY as such planes (column ranges as in pxr_attn_bwd_f32) + the 64 spread maxima.
 * pxr_h2_sites_update: n <= 16 sites; per site m = max(maximum of its n_parts[s] partial maxima, run_max[s] * decay) (the maxima are
 *   heavy-tailed: the scale follows a decaying maximum of the recent steps; run_max persistent, zero-initialised) -> exps[s] (m 2^e in
 *   [2^(13-headroom), 2^(14-headroom))), stats[2 s ..] = (max 2^headroom, rows[s] max 2^headroom) and, where bound_b[s] (the largest
 *   column sum of |W| of the weight behind the site) is given, bexp[s] = 15 - ceil(log2(max 2^headroom * bound_b[s][0] * bound_factor)):
 *   the exponent of the planes a GEMM epilogue writes from site s (pxr_h2_bound_exp's rule).  A site without gradient keeps its entries.
 *   Run it once per step after the LAST reader of the site exponents; seed it with one exact pass (pxr_ln_bwd_stat_f32 /
 *   pxr_attn_bwd_stat_f32 + pxr_h2_split_parts_f32 leave the same partial maxima). */
int pxr_ln_bwd_h2s_f32(const float* pos_score, const float* neg_score, const float* table, int64_t n_table, const int64_t* items,
                       const int64_t* masked_index, int B, int L, float grad_scale, const float* grad_scale_dev, float* coef,
                       const float* dy, const float* xhat, const float* rstd, const float* gamma, int rows, int D, float* dz,
                       float* dgamma, float* dbeta, float p_drop, uint64_t seed, uint32_t stream_id, const int64_t* step_dev,
                       void* ws, int64_t ws_bytes, void* g_planes, int64_t g_plane_stride, int64_t g_panel_rows,
                       const int* g_exp_dev, float* stat, float* zero, int zero_n, int64_t id_bstride, int64_t pos_off,
                       int64_t neg_off, void* stream);
int pxr_attn_bwd_h2s_f32(const float* dctx, int64_t ld_ctx, const float* q, const float* k, const float* v, int64_t ld,
                         const float* probs, int B, int H, int L, int d, float p_drop, uint64_t seed, uint32_t stream_id,
                         const int64_t* step_dev, void* g_planes, int64_t g_plane_stride, int64_t g_panel_rows, int g_cols,
                         int col_q, int col_k, int col_v, const int* g_exp_dev, float* stat, void* stream);
int pxr_h2_sites_update(int n, const float* const* parts, const int* n_parts, const int* rows, const float* const* bound_b,
                        float bound_factor, int headroom, float decay, float* run_max, int* exps, float* stats, int* bexp, void* stream);

/* Producers that write their output straight as planes: pxr_input_ln_fwd_f32 / pxr_ln_residual_fwd_f32 (y), pxr_ln_bwd_f32
 * (residual sites: the gradient the next GEMMs read, dx when given, else dz), pxr_attn_fwd_f32 (ctx as the [B*L, H*d] matrix;
 * ctx may then be NULL), pxr_attn_bwd_f32 (dq | dk | dv as column ranges starting at col_q / col_k / col_v of one [B*L, g_cols]
 * matrix; dq, dk, dv may then all be NULL), pxr_adamw_flat_tab_f32 and pxr_score_topk_f32 (pre-split operands); planes NULL:
 * fp32 outputs only.  pxr_attn_planes_supported(L, d): whether the fused attention kernels that can do so serve the shape. */
int pxr_attn_planes_supported(int L, int d);
/* Measurement hook of bench.py (no reference analogue): registers two uint64 in DEVICE memory (NULL unregisters).  Every later
 * main-pass launch of the fused scoring's DEFAULT (reduced-product) threshold kernel adds the shader-clock cycles (s_memtime) and the constant 100 MHz reference ticks
 * (s_memrealtime) that its workgroup 0 lived through: clk2[0] / clk2[1] * 0.1 = the clock in GHz the part sustained INSIDE those
 * kernels (it lowers its clock under MFMA load; the nominal 2.4 GHz is what the 2.5 PFLOP/s peak assumes).  The caller zeroes the
 * buffer.  Process-wide; replaces round 5's pxr_clock_probe_f32 (a one-wave probe on a second stream, which read the idle clock). */
int pxr_score_topk_clock_out(uint64_t* clk2);
/* Host-side recovery after PXR_STATUS_GEMM_TIMEOUT (a stream-K / split-K worker gave up waiting for a partial tile): waits for
 * the device and zeroes every stream's flag words, so that later launches start from the state they expect.  No reference
 * analogue: this build's own synchronisation (gemm_f32.hip stream-K, gemm_p3.hip split-K weight gradients). */
int pxr_gemm_reset_flags(void);
/* pxr_grouped_linear_bwd_weight_f32 from planes: dW[i][N_i,K_i] = dy[i][T_i,N_i]^T x[i][T_i,K_i], db[i][N_i] = column sums
 * of dy[i] (db[i] may be NULL), all problems in one launch.  dy[i] / x[i] are planes of the [T_i, .] matrices whose panel
 * rows (multiples of 32) T_i .. panel_rows-1 are ZERO.  N_i, K_i multiples of 32.  Autograd of model/layers.py:586-588,613,
 * 666,669. */
int pxr_grouped_dw_planes_f32(int n, const void* const* dy, const int64_t* dy_plane_stride, const int64_t* dy_panel_rows,
                              const void* const* x, const int64_t* x_plane_stride, const int64_t* x_panel_rows,
                              float* const* dW, float* const* db, const int* T, const int* N, const int* K, int tile_hint,
                              void* stream);

/* ---- ViT image encoder, non-GEMM pieces (csrc/vit.hip) ------------------------------------------------------ */
/* Fused self-attention of a tower block, forward (csrc/tower_attn.hip): per (image, head)
 * ctx[b*T + t, 64 h ..] = softmax_t'(scale * q_t . k_t') v_t'; no mask, no dropout (HF CLIPAttention.forward as the item tower of
 * REC/model/modules.py runs it).  q/k/v fp32, element (b, t, h, c) at p[(b*T + t)*ld + 64 h + c]; head size 64, T <= 288
 * (pxr_tower_attn_supported).  Outputs: ctx fp32 [images*T, ld_ctx] and/or ctx as planes (at least one; planes_fmt 0 = bf16x3,
 * 1 = h2); lse (optional) [images*heads, T] = log sum_t' exp(scale * q.k).  The score matrix never exists in memory. */
int pxr_tower_attn_supported(int T, int d);
int pxr_tower_attn_fwd_f32(const float* q, const float* k, const float* v, int64_t ld, int64_t images, int heads, int T, int d,
                           float scale, float* ctx, int64_t ld_ctx, void* ctx_planes, int64_t ctx_plane_stride,
                           int64_t ctx_panel_rows, int planes_fmt, float* lse, void* stream);
/* Backward of pxr_tower_attn_fwd_f32 (the trainable blocks of the tower): dq | dk | dv from dctx, recomputing the
 * probabilities from the forward's lse -- no [images*heads, T, T] matrix is saved or written.  ctx = the forward's fp32
 * output (for delta = rowsum(dctx o ctx)); delta_ws = [images*heads, T] floats of scratch; dq / dk / dv are addressed like
 * q / k / v with row stride ld_d (three column ranges of one [images*T, 3*heads*64] matrix in the tower).  Two launches. */
int pxr_tower_attn_bwd_f32(const float* q, const float* k, const float* v, int64_t ld, const float* dctx, const float* ctx,
                           int64_t ld_c, const float* lse, int64_t images, int heads, int T, int d, float scale, float* dq,
                           float* dk, float* dv, int64_t ld_d, float* delta_ws, void* stream);
/* in place: S[row, :T] = softmax(scale * S[row, :T]), S[row, T:ld] = 0      (HF CLIPAttention, no mask / dropout) */
int pxr_softmax_rows_f32(float* S, int64_t rows, int T, int ld, float scale, void* stream);
/* in place on dP: dS = scale * P o (dP - rowsum(dP o P))                    (autograd of the above) */
int pxr_softmax_rows_bwd_f32(const float* P, float* dP, int64_t rows, int T, int ld, float scale, void* stream);
/* out[n,t,:] = (t == 0 ? cls : patches[n,t-1,:]) + pos[t,:]                (HF CLIPVisionEmbeddings.forward) */
int pxr_vit_embed_f32(const float* patches, const float* cls, const float* pos, float* out, int64_t n, int T, int H,
                      void* stream);
/* out[n,:] = mean_t x[n,t,:]                                                (MeanItemEncoder, model/layers.py:128) */
int pxr_token_mean_f32(const float* x, float* out, int64_t n, int T, int D, void* stream);
/* dact[n,t,:] = act[n,t,:] > 0 ? dout[n,:] / T : 0                          (through the mean and rec_fc's ReLU) */
int pxr_token_mean_relu_bwd_f32(const float* dout, const float* act, float* dact, int64_t n, int T, int D, void* stream);
/* SASRec attention for MAX_ITEM_LIST_LENGTH > 128 (beyond the fused kernels behind pxr_attn_fwd_f32): the scores come
 * from a batched GEMM (S = Q K^T, unscaled, [B*H, L, ld]); this turns them in place into softmax(S / sqrt(d) + mask) with
 * the reference's additive -1e9 causal + key mask (model/layers.py:595-604, model/IDNet/sasrec.py:119-126) and writes
 * the dropped probabilities (layers.py:608; same counter hash and element numbering as pxr_attn_fwd_f32) to PD.  causal = 0:
 * the key-padding mask only (BERT4Rec, bert4rec.py:150-155). */
int pxr_attn_rows_fwd_f32(float* S, float* PD, const int64_t* keymask, int64_t km_bstride, int B, int H, int L, int ld,
                          float p_drop, uint64_t seed, uint32_t stream_id, const int64_t* step_dev, int d, int causal,
                          void* stream);
/* in place on dPD (gradient w.r.t. the dropped probabilities): gradient w.r.t. the unscaled scores (either mask) */
int pxr_attn_rows_bwd_f32(const float* P, float* dPD, int B, int H, int L, int ld, float p_drop, uint64_t seed,
                          uint32_t stream_id, const int64_t* step_dev, int d, void* stream);
/* out = a + b (n floats, n % 4 == 0): the two branches of a residual-stream gradient */
int pxr_add_f32(const float* a, const float* b, float* out, int64_t n, void* stream);
/* y = dropout(x): y[i] = x[i] / (1 - p) where the library's counter hash of (seed + *step_dev, stream_id, i) keeps element i, else
 * 0 (n floats, n % 4 == 0, 16-byte aligned; step_dev may be NULL).  Applied to the upstream gradient it is its own backward: the
 * mask is regenerated, not stored.  Replaces nn.Dropout on the gathered item embeddings of GRU4Rec
 * (REC/model/IDNet/gru4rec.py:26,59); masks restated for the oracle in oracle/dropout_rng.py. */
int pxr_dropout_f32(const float* x, float* y, int64_t n, float p, uint64_t seed, uint32_t stream_id, const int64_t* step_dev,
                    void* stream);

/* y = x W^T + b (act=1: erf-GELU, pre-activation saved; act=2: erf-GELU, gelu'(pre-activation) saved; act=3..7: relu / swish /
 * tanh / sigmoid / selu of it, act'(pre-activation) saved -- selu' at exactly 0 is scale * alpha, torch's backward)
 *                                        layers.py:586-588,613,642-649,666-667,669; sasrec.py:112; ViNet/curatornet.py:67-82 */
int pxr_linear_fwd_f32(const float* x, const float* W, const float* b, float* y, float* pre, int M, int N, int K,
                       int act, void* stream);
/* dx = dy W, optionally * gelu'(dgelu_pre) OR + add (residual gradient) OR * mul (gelu' saved by act=2);
 * dW = dy^T x  -- autograd of nn.Linear */
int pxr_linear_bwd_input_f32(const float* dy, const float* W, float* dx, const float* dgelu_pre, const float* add,
                             const float* mul, int M, int N, int K, void* stream);
int pxr_linear_bwd_weight_f32(const float* dy, const float* x, float* dW, int M, int N, int K, void* ws,
                              int64_t ws_bytes, void* stream);
/* Weight AND bias gradients of up to 16 nn.Linear layers in ONE launch (host arrays of n device pointers / sizes):
 * dW[i][N_i,K_i] = dy[i][M_i,N_i]^T x[i][M_i,K_i], db[i][N_i] = column sums of dy[i] (db[i] may be NULL).
 * No split-K, no partial buffers: all problems' 64x64 tiles share one grid.  Deterministic. */
int pxr_grouped_linear_bwd_weight_f32(int n, const float* const* dy, const float* const* x, float* const* dW,
                                      float* const* db, const int* M, const int* N, const int* K, void* stream);
/* out[n] = sum_m x[m,n]  (bias grads; position-embedding grad = colsum of dx0 viewed [B, L*D]); deterministic */
int64_t pxr_colsum_ws_bytes(int M, int N);
int pxr_colsum_partial_rows(int M);      /* rows of the [P, N] partial buffer left in ws when out is NULL */
/* out_a[i][c] (c < split[i]) / out_b[i][c-split[i]] = sum_p part[i][p][c] for up to 16 partial buffers in one launch
 * (host arrays of n entries; out_b[i] may be NULL => single output).  bump_counter (optional): a device counter
 * incremented by one by the same launch (the dropout step counter at the end of a backward pass). */
int pxr_reduce_partials_multi_f32(int n, const float* const* part, const int* P, const int* N, float* const* out_a,
                                  float* const* out_b, const int* split, int64_t* bump_counter, void* stream);
int pxr_colsum_f32(const float* x, int64_t ldx, int M, int N, float* out, void* ws, int64_t ws_bytes, void* stream);

/* ---- masked multi-head self-attention core ------------------------------------------------------------------ */
/* ctx = softmax(q k^T / sqrt(d) + mask) v with the reference's additive -1e9 causal+padding mask
 * (layers.py:590-612, sasrec.py:119-126).  q/k/v element (b,t,h,c) at p[(b*L+t)*ld + h*d + c] (fused QKV output);
 * key j of batch b is real iff keymask[b*km_bstride + j] != 0 (masked_index in training, item_seq in predict).
 * ctx is written head-merged [B*L, ld_ctx]; probs [B,H,L,L] (pre-dropout) is saved for backward, may be NULL.  ctx planes:
 * "Producers that write their output straight as planes" (planes_fmt 0 = bf16x3, 1 = h2).  causal = 0: the key-padding mask
 * only, -1e9 on keys whose keymask entry is 0, no causal term (BERT4Rec, bert4rec.py:150-155).  The backward serves both masks:
 * it works from the saved probabilities. */
int pxr_attn_fwd_f32(const float* q, const float* k, const float* v, int64_t ld, const int64_t* keymask,
                     int64_t km_bstride, int B, int H, int L, int d, float* ctx, int64_t ld_ctx, float* probs,
                     float p_drop, uint64_t seed, uint32_t stream_id, const int64_t* step_dev, void* ctx_planes,
                     int64_t ctx_plane_stride, int64_t ctx_panel_rows, int planes_fmt, int causal, void* stream);
int pxr_attn_bwd_f32(const float* dctx, int64_t ld_ctx, const float* q, const float* k, const float* v, int64_t ld,
                     const float* probs, int B, int H, int L, int d, float* dq, float* dk, float* dv, int64_t ld_d,
                     float p_drop, uint64_t seed, uint32_t stream_id, const int64_t* step_dev, void* g_planes,
                     int64_t g_plane_stride, int64_t g_panel_rows, int g_cols, int col_q, int col_k, int col_v, void* stream);

/* ---- GRU4Rec (code/REC/model/IDNet/gru4rec.py; torch.nn.GRU, bias=False): the gate arithmetic of one time step --------- */
/* r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n), h = (1 - z) n + z h_prev; gi, gh [B, 3H] in
 * torch's r | z | n order, h_prev [B, H] or NULL (zeros), save (optional) [B, 4H] = r | z | n | gh_n.  The matrix products
 * around it are pxr_linear_* / pxr_gemm_f32 calls. */
int pxr_gru_gates_fwd_f32(const float* gi, const float* gh, const float* h_prev, float* h_out, float* save, int64_t B, int H,
                          void* stream);
/* dh = everything that reaches h_t  ->  dgi, dgh [B, 3H] and the direct part dh * z of d h_{t-1} (autograd of the above) */
int pxr_gru_gates_bwd_f32(const float* dh, const float* save, const float* h_prev, float* dgi, float* dgh, float* dh_prev,
                          int64_t B, int H, void* stream);

/* ---- NextItNet (code/REC/model/IDNet/nextitnet.py:160-194): the causal dilated convolution as a GEMM ------------------ */
/* xcol[b L + t, c k + j] = x[b, t - (k-1-j) dilation, c] (0 left of the sequence): conv = xcol . W.view(C_out, C_in k)^T + bias
 * with the reference's Conv2d weight [C_out, C_in, 1, k] used in place.  col2im is its transpose (the input gradient). */
int pxr_causal_im2col_f32(const float* x, float* xcol, int64_t B, int L, int C, int k, int dilation, void* stream);
int pxr_causal_col2im_f32(const float* dxcol, float* dx, int64_t B, int L, int C, int k, int dilation, void* stream);

/* ---- training head ------------------------------------------------------------------------------------------ */
/* loss = mean_b(-sum_t log(sigmoid(pos-neg)+1e-8) * mask)            sasrec.py:88-92; loss stays on the device
 * The id layout: position t of sequence b scores against items[b*id_bstride + pos_off + t] (target) and
 * items[b*id_bstride + neg_off + t] (negative).  SASRec's shifted windows items [B, 2, L+1] are (2(L+1), 1, L+2).  BERT4Rec's
 * batch items [B, 3, L] = masked sequence | original sequence | negatives over its L = MAX_ITEM_LIST_LENGTH + 1 positions
 * (REC/data/dataset/trainset.py:470-478) is (3L, L, 2L), with masked_index [B, L]: the loss -sum_masked log(1e-8 +
 * sigmoid(pos - neg)) / B of bert4rec.py:98-111 is this function on that layout. */
int pxr_bpr_loss_fwd_f32(const float* out, const float* table, int64_t n_table, const int64_t* items,
                         const int64_t* masked_index, int B, int L, int D, float* pos_score, float* neg_score,
                         float* lossrow, float* loss, int64_t id_bstride, int64_t pos_off, int64_t neg_off, void* stream);
int pxr_bpr_loss_bwd_f32(const float* pos_score, const float* neg_score, const float* table, int64_t n_table,
                         const int64_t* items, const int64_t* masked_index, int B, int L, int D, float grad_scale,
                         const float* grad_scale_dev, float* dout, float* coef, int64_t id_bstride, int64_t pos_off,
                         int64_t neg_off, void* stream);
/* The block's LAST LayerNorm (reference layers.py:670-671, the output sasrec.py:86 names) with the loss head's forward
 * (sasrec.py:88-92) fused in: y = LN(dropout(x) + res) over B*L rows, pos / neg scores and the loss as pxr_bpr_loss_fwd_f32
 * would compute them from y -- bit-identical, one launch and one pass over y less.  Same id layout.  loss == NULL: lossrow is
 * written and the one-workgroup sum over it is left to the caller (a pxr_tail_rider of the same step's backward). */
int pxr_ln_residual_bpr_fwd_f32(const float* x, const float* res, const float* gamma, const float* beta, float eps, int B, int L,
                                int D, float* y, float* xhat, float* rstd, float p_drop, uint64_t seed, uint32_t stream_id,
                                const int64_t* step_dev, const float* table, int64_t n_table, const int64_t* items,
                                const int64_t* masked_index, float* pos_score, float* neg_score, float* lossrow, float* loss,
                                int64_t id_bstride, int64_t pos_off, int64_t neg_off, void* stream);
/* Its backward: pxr_bpr_loss_bwd_f32 + pxr_ln_bwd_f32 (gather_mode 0) in one launch -- the gradient w.r.t. the block's
 * output is formed per row in registers from the saved scores instead of being written and read back; coef [B*L] is written
 * for pxr_sasrec_occ_segsum.  g_planes / stat optional (the two forms of pxr_ln_bwd_f32 / pxr_ln_bwd_stat_f32). */
int pxr_bpr_ln_bwd_f32(const float* pos_score, const float* neg_score, const float* table, int64_t n_table, const int64_t* items,
                       const int64_t* masked_index, int B, int L, float grad_scale, const float* grad_scale_dev, float* coef,
                       const float* xhat, const float* rstd, const float* gamma, int D, float* dz, float* dx, float* dgamma,
                       float* dbeta, float p_drop, uint64_t seed, uint32_t stream_id, const int64_t* step_dev, void* ws,
                       int64_t ws_bytes, void* g_planes, int64_t g_plane_stride, int64_t g_panel_rows, float* stat,
                       int64_t id_bstride, int64_t pos_off, int64_t neg_off, void* stream);

/* ---- PixelNet (MOSASRec) ------------------------------------------------------------------------------------- */
/* Gradient w.r.t. the visual encoder's output viewed [B, L+1, 2, D] (pos_t | neg_t interleaved, PixelNet/
 * mosasrec.py:69-74,88-89): d_emb[b,t,0] = [t<L] dx0[b,t] + [t>=1] coef[b,t-1] out[b,t-1];  d_emb[b,t,1] = -[t>=1] ... */
int pxr_mosasrec_emb_grad_f32(const float* dx0, const float* out, const float* coef, int B, int L, int D, float* d_emb,
                              void* stream);
/* The reference's image transform on the GPU (data/dataset/trainset.py:85-96): uint8 HWC store [n_store,H,W,3] gathered
 * by item id -> fp32 [n,3,H,W] = (x/255 - 0.5)/0.5; id 0 (padding) -> zeros.  An id outside [0, n_store) -> zeros too
 * (nothing is read) and PXR_STATUS_BAD_INDEX in the status word of pxr_set_status_word. */
int pxr_image_u8_to_f32(const uint8_t* store, int64_t n_store, int H, int W, const int64_t* ids, int n, float* out,
                        void* stream);

/* ---- full-sort evaluation ------------------------------------------------------------------------------------ */
/* Fused  scores = users x table^T (sasrec.py:112)  ->  scores[:,0] = -inf, scores[history] = -inf (trainer.py:333-336)
 * ->  top-K (collector.py:133): the [B,N] score matrix never reaches HBM.  users [B,D] with row stride ld_users;
 * hist_ptr int32 [B+1] + hist_items int64 = CSR of seq_eval_collate's (history_u, history_i) pairs (NULL = none);
 * K <= 32.  Outputs topk_idx int64 [B,K] / topk_val [B,K], descending. */
int64_t pxr_score_topk_ws_bytes(int B, int N, int K);
/* users_planes / table_planes: both operands ALSO given as planes ("pre-split operands" above; both NULL: fp32 only): on
 * catalogues that take the two-pass threshold schedule the pass over every item tile runs on the planes as one LDS-DMA stream;
 * the table's planes are made once per evaluation with pxr_split_planes_f32 (model/IDNet/sasrec.py:112,115-117).  That pass
 * runs on `products` = 6, 3 (hi*hi + mid*hi + hi*mid) or 1 (hi*hi) of the six bf16 products; it only decides "score >=
 * threshold": with 3 or 1 the threshold is lowered by a rigorous per-user bound on what the dropped products and the different
 * rounding can change (c ||user||_2 max_i ||table[i]||_2), and the few survivors that can still reach the top K are re-scored
 * with all six products in the full pass's own MFMA order -- ids and values are the six-product pass's, bit for bit, at about
 * half (3) of its MFMA work.  products 3 / 1 need both operands as planes and table_row_norm_max: DEVICE pointer to
 * max_i ||table[i]||_2 (pxr_row_norm_max_f32, once per evaluation like the planes; NULL with 6).
 * Same reference path: model/IDNet/sasrec.py:112 + trainer/trainer.py:327-337 + evaluator/collector.py:131-139. */
int pxr_score_topk_f32(const float* users, int64_t ld_users, int B, const float* table, int N, int D,
                       const void* users_planes, int64_t users_plane_stride, int64_t users_panel_rows,
                       const void* table_planes, int64_t table_plane_stride, int64_t table_panel_rows,
                       const float* table_row_norm_max, int products, const int32_t* hist_ptr, const int64_t* hist_items,
                       int K, int64_t* topk_idx, float* topk_val, void* ws, int64_t ws_bytes, void* stream);
/* out[0] (device float) = max_i ||x[i, :]||_2 of x [rows, cols] fp32 (row stride ldx, cols % 4 == 0): the item-table statistic of
 * the function above (computed over what compute_item_all returns, model/IDNet/sasrec.py:115-117). */
int pxr_row_norm_max_f32(const float* x, int64_t rows, int64_t cols, int64_t ldx, float* out, void* stream);

/* ---- optimizer ---------------------------------------------------------------------------------------------- */
/* torch.optim.AdamW update (trainer.py:102,125), step is 1-based.  n must be a multiple of 4. */
int pxr_adamw_flat_f32(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1,
                       double beta2, double eps, double weight_decay, int64_t step, void* stream);
/* Dense-semantics AdamW over the whole table with the gradient given sparsely; slot is an int32[N] map that must be
 * all -1 on entry (pxr_slot_fill_i32 once) and is all -1 again on exit. */
int pxr_slot_fill_i32(int32_t* slot, int64_t n, int32_t value, void* stream);
int pxr_adamw_table_f32(float* table, float* m, float* v, int64_t n_rows, int D, int32_t* slot,
                        const int64_t* uniq_idx, const float* uniq_rows, const int32_t* n_uniq_dev, int64_t max_uniq,
                        double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                        void* stream);

/* Lazy (exact catch-up) form of the same dense-semantics table update: no O(N*D) sweep per step.  last int32[N]
 * holds, per row, the optimizer step through which the row is up to date; hyper (float4[capacity]) / cumlog
 * (double[capacity]) hold each step's scalars, appended once per step.  pxr_adamw_rows_f32 replays a row's missed
 * zero-gradient steps (bit-identical to the sweep for gaps <= 256 steps, closed-form weight decay beyond) through
 * t_prev and, if t_apply = t_prev+1, applies that step with gradient rows grows[i,:].  rows == NULL: all N rows
 * (flush before evaluation / checkpointing).  With step_dev the kernel takes t_prev = *step_dev + step_dev_bias from the
 * device (bias 1 = "through the step being applied": the rows of the NEXT batch, prefetched); max_blocks > 0 caps the
 * grid (a thin launch that shares the CUs with the step's GEMMs instead of flooding them).  hyper_append with advance != 0 is the end-of-step form: it first counts
 * the finished step (*step_dev += 1) and then appends the scalars of the next one, in one launch. */
int pxr_adamw_hyper_append(void* hyper, void* cumlog, int64_t capacity, int64_t step, int64_t* step_dev,
                           double lr, double beta1, double beta2, double eps, double weight_decay, int advance,
                           void* stream);
int pxr_adamw_rows_f32(float* table, float* m, float* v, int32_t* last, int64_t n_table, int D, const int64_t* rows,
                       const int32_t* n_rows_dev, int64_t max_rows, const float* grows, const void* hyper,
                       const void* cumlog, int64_t t_prev, int64_t t_apply, const int64_t* step_dev,
                       int64_t step_dev_bias, int64_t max_blocks, double beta1, double beta2, double eps,
                       void* stream);
/* The catch-up part of pxr_adamw_rows_f32 on a RAW id list (the batch's item tensor as it is): ids[n_ids] may hold
 * duplicates, 0 and out-of-range values (skipped).  The workgroup that raises last[row] to t_prev (atomicMax) replays the
 * row, the ones of its duplicates find it current -- so the rows a forward pass reads can be brought up to date BEFORE the
 * sort / unique of the batch's ids has run (it then runs beside the forward pass on a second stream). */
int pxr_adamw_rows_ids_f32(float* table, float* m, float* v, int32_t* last, int64_t n_table, int D, const int64_t* ids,
                           int64_t n_ids, const void* hyper, const void* cumlog, int64_t t_prev, const int64_t* step_dev,
                           double beta1, double beta2, double eps, void* stream);
/* The same over a 2-D window of an id tensor: n_lists rows of row_len ids, row r at ids[r * row_stride] -- the INPUT ids
 * items[:, 0, 0:L] of a batch [B, 2, L+1] (reference sasrec.py:68-70: the rows the forward pass gathers first), so that only
 * those rows stand between the batch and the first LayerNorm; the targets / negatives (read by the loss, sasrec.py:88-89) are
 * caught up beside the forward pass (pixelrec_amd/model/sasrec.py "split catch-up"). */
int pxr_adamw_rows_ids2d_f32(float* table, float* m, float* v, int32_t* last, int64_t n_table, int D, const int64_t* ids,
                             int64_t n_lists, int64_t row_len, int64_t row_stride, const void* hyper, const void* cumlog,
                             int64_t t_prev, const int64_t* step_dev, double beta1, double beta2, double eps,
                             void* cur_hyper_out, void* stream);
/* cur_hyper_out (optional, 16 bytes): the launch also copies the scalars of the optimizer step about to run (hyper entry
 * t_prev + 1) there.  pxr_adamw_flat_tab_ex_f32 = pxr_adamw_flat_tab_f32 with two options: (a) seg_fmt = 1: the weight
 * segments leave the launch as fp16 two-plane operands (planes "h2"), segment i scaled by 2^seg_exps[i] (device ints: the
 * exponents the planes were last split with; the next forward needs no statistics + split launches); (b) cur_hyper != NULL: this
 * step's scalars are read from that slot and the launch CLOSES the step itself (counts it in *step_dev, appends the next entry:
 * what pxr_adamw_hyper_append(advance = 1) does in a launch of its own) -- legal because no workgroup of the launch reads the
 * counter its closing thread advances.  Reference: torch.optim.AdamW.step (trainer.py:125). */
int pxr_adamw_flat_tab_ex_f32(float* p, const float* g, float* m, float* v, int64_t n, void* hyper, void* cumlog, int64_t capacity,
                              int64_t step, int64_t* step_dev, const void* cur_hyper, double lr, double beta1, double beta2,
                              double eps, double weight_decay, int n_seg, const int64_t* seg_off, const int64_t* seg_rows,
                              const int64_t* seg_cols, void* const* seg_planes, const int64_t* seg_plane_stride,
                              const int64_t* seg_panel_rows, int seg_fmt, const int* seg_exps, void* stream);
/* pxr_adamw_flat_f32 with the step's scalars read from hyper[step] (or hyper[*step_dev + 1]); it also writes the UPDATED values
 * of n_seg (<= 16; 0: none) weight matrices inside the flat buffer ([seg_rows, seg_cols] row-major at element seg_off) as bf16x3
 * planes (see "pre-split operands"): the operands of the next step's GEMMs come out of the optimizer (trainer.py:125) with no
 * split launch. */
int pxr_adamw_flat_tab_f32(float* p, const float* g, float* m, float* v, int64_t n, const void* hyper, int64_t step,
                           const int64_t* step_dev, double beta1, double beta2, double eps, int n_seg,
                           const int64_t* seg_off, const int64_t* seg_rows, const int64_t* seg_cols,
                           void* const* seg_planes, const int64_t* seg_plane_stride, const int64_t* seg_panel_rows,
                           void* stream);
/* *counter += delta on the device. */
int pxr_counter_add_i64(int64_t* counter, int64_t delta, void* stream);

/* ---- LightGCN (model/IDNet/lightgcn.py, layers.py:13-22; csrc/lightgcn.hip) ----------------------------------------------- */
/* CSR SpMM over the symmetric normalised user-item graph with a fused layer-mean epilogue: s = A x (row_ptr int64 [n_rows+1],
 * col int32 / w fp32 [nnz], x [n_rows, D]); y = s when y is given; acc_out = (acc_in + s) * scale when acc_out is given (acc_in
 * may be NULL: 0, and may equal acc_out).  x must not alias y or acc_out.  Rows of more than part_len edges are the n_split rows
 * split_row[j], cut into parts of part_len edges (parts split_part0[j] .. split_part0[j+1]-1, n_parts in all, part_owner[q] = j)
 * that are summed in part order: deterministic, no atomics.  A neighbour id outside [0, n_rows) ORs bit 0 into the status word
 * (clamped).  D % 4 == 0, D <= 2048.  ws: pxr_lgcn_spmm_ws_bytes(n_parts, D). */
int64_t pxr_lgcn_spmm_ws_bytes(int64_t n_parts, int D);
int pxr_lgcn_spmm_f32(const int64_t* row_ptr, const int32_t* col, const float* w, int64_t n_rows, int D,
                      const int32_t* split_row, const int32_t* split_part0, int n_split, const int32_t* part_owner,
                      int n_parts, int part_len, const float* x, float* y, const float* acc_in, float* acc_out,
                      float scale, void* ws, int64_t ws_bytes, void* stream);
/* Pair loss head (lightgcn.py:70-78) on E_final [n_users + n_items, D] (users first): x_b = <u_b, i+_b> - <u_b, i-_b> with
 * user[b] and item[b, 0..1] = (positive, negative); lossrow[b] = -(1e-8 + log sigmoid(x_b)), loss = mean, coef[b] =
 * d loss / d x_b = -(1 - sigmoid(x_b)) / B, nodes[3b..3b+2] = the three row ids (int32).  Ids outside [0, n_users) /
 * [0, n_items) OR bit 0 into the status word (clamped). */
int pxr_lgcn_pair_fwd_f32(const float* emb, int64_t n_users, int64_t n_items, int D, const int64_t* user,
                          const int64_t* item, int B, float* diff, float* coef, float* lossrow, int32_t* nodes,
                          float* loss, void* stream);
/* Its backward: grad [n_nodes, D] is zeroed, then every row the batch touched gets the sum of its contributions in occurrence
 * order (deterministic when users and items repeat); upstream d(loss) = grad_scale * (*grad_scale_dev if given). */
int pxr_lgcn_pair_bwd_f32(const float* emb, int64_t n_nodes, int D, const int32_t* nodes, const float* coef, int B,
                          float grad_scale, const float* grad_scale_dev, float* grad, void* stream);

/* ---- SRGNN (model/IDNet/srgnn.py, collate_fn.py graph_train_collate; csrc/srgnn.hip) ----------------------------------------- */
/* Session graphs built on the device at a FIXED size of L nodes (the collate pads to the batch's largest node count): one wave per
 * sequence seq [B, L] (right-padded with 0).  nodes [B, L] = the distinct ids ascending (0 included when padded), then 0;
 * alias [B, L] = node index of seq[b, t]; A [B, L, 2L] = [A_in | A_out] with A_in[v][u] = e(u,v) / indeg(v), A_out[u][v] =
 * e(u,v) / outdeg(u) (a degree of 0 counts as 1), edges seq[i] -> seq[i+1] until the next id is 0, a repeat counted once.
 * Optional: occ [B, 3L] = nodes | target[b,0], 0.. | target[b,1], 0.. (the id rows of pxr_seq_occ_sort with layout (3L, 0, L,
 * 2L); needs target [B, 2]); mask [B, L] = seq != 0.  An id outside [0, n_items) ORs bit 0 into the status word (clamped).
 * 1 <= L <= 64. */
int pxr_srgnn_graph_i64(const int64_t* seq, int64_t B, int L, int64_t n_items, const int64_t* target, int64_t* nodes,
                        int32_t* alias, float* A, int64_t* occ, int64_t* mask, void* stream);
/* One workgroup per session, A in LDS; x, y [B*L, 2D].  transpose 0: y[v] = [sum_u A_in[v][u] x[u, :D] | sum_u A_out[v][u]
 * x[u, D:]] + bias (bias [2D] or NULL); transpose 1 (the backward, no bias): y[u] = [sum_v A_in[v][u] x[v, :D] | sum_v
 * A_out[v][u] x[v, D:]].  Sums in ascending node order.  D % 4 == 0, D <= 2048, L <= 64. */
int pxr_srgnn_prop_f32(const float* A, int B, int L, int D, const float* x, float* y, const float* bias, int transpose,
                       void* stream);
/* Readout (srgnn.py seq_modeling after the GNN), one workgroup per session.  Hn [B*L, D] node states, P [B*L, 2D] = [Hn W1^T
 * + b1 | Hn W2^T + b2]; position t reads node alias[b, t]; last = sum(mask[b]) - 1 (an empty history wraps to L-1 like torch
 * indexing).  s_t = sigmoid(P1[last node] + P2[alias t]), alpha_t = <w3, s_t>, cat [B, 2D] = [sum_t alpha_t sh_t mask_t | ht].
 * sig [B, L, D] / alpha [B, L] are saved for the backward (may be NULL for inference). */
int pxr_srgnn_readout_fwd_f32(const float* Hn, const float* P, const int32_t* alias, const int64_t* mask, const float* w3,
                              int B, int L, int D, float* cat, float* sig, float* alpha, void* stream);
/* Its backward from dcat [B, 2D]: dP [B*L, 2D], dH [B*L, D] (the direct paths into the node states) and dw3p [B, D] (per-session
 * parts of d w3, reduced by pxr_colsum_f32).  A node's sums run over its positions in ascending order: no atomics. */
int pxr_srgnn_readout_bwd_f32(const float* dcat, const float* Hn, const int32_t* alias, const int64_t* mask, const float* w3,
                              const float* sig, const float* alpha, int B, int L, int D, float* dP, float* dH, float* dw3p,
                              void* stream);
/* Pair loss head (srgnn.py:60-66): x_b = <out_b, e[target b,0]> - <out_b, e[target b,1]> with out rows ld_out floats apart;
 * lossrow[b] = -(1e-8 + log sigmoid(x_b)), loss = mean, coef[b] = -(1 - sigmoid(x_b)) / B.  Ids outside [0, n_table) OR bit 0
 * into the status word (clamped). */
int pxr_srgnn_pair_fwd_f32(const float* out, int64_t ld_out, const float* table, int64_t n_table, int D, const int64_t* target,
                           int B, float* lossrow, float* coef, float* loss, void* stream);
/* Its backward: c_b = coef[b] * grad_scale * (*grad_scale_dev if given); dout[b] = c_b (e[pos] - e[neg]) (rows ld_dout apart);
 * coef_out[b * coef_stride] = c_b (optional) for the target rows' gradient in pxr_sasrec_occ_segsum. */
int pxr_srgnn_pair_bwd_f32(const float* table, int64_t n_table, int D, const int64_t* target, const float* coef, int B,
                           float grad_scale, const float* grad_scale_dev, float* dout, int64_t ld_dout, float* coef_out,
                           int64_t coef_stride, void* stream);

/* ---- LightSANs (model/IDNet/lightsans.py; model/layers.py:762-932 ItemToInterestAggregation / LightMultiHeadAttention; ------ */
/* ---- csrc/lightsans.hip).  One workgroup per sequence; fp32 throughout, no float atomics, sums in a fixed order.  Limits:   */
/* ---- 1 <= L <= 64, D <= 1024 with D % (4H) == 0, 1 <= K <= 16 (anything else fails with a message).                        */
/* Forward core (layers.py:784-790, 839-878 up to the merged context), no mask anywhere.  qkv [B*L, 3D] = q | k | v rows;
 * theta [2, D, K] = attpooling_key.theta | attpooling_value.theta; A [H, L, L] = the position probabilities.
 * pi_K = softmax over l of (k thK), Kp = pi_K^T k (Vp from v and thV); per head S = q_h Kp_h^T / sqrt(dh), P = softmax over the
 * QUERIES (dim -2), P~ = dropout(P) with keep(seed + *step_dev, stream_id, ((b H + h) L + i) K + k) (the counter hash of
 * pxr_dropout_f32, scaled 1/(1-p)); ctx [B*L, D] (head-merged) = P~ Vp_h + A_h v_h.  KVp [B, 2K, D] = Kp rows then Vp rows
 * (always written); pi [B, 2, L, K] (pi_K | pi_V) and probs [B, H, L, K] (P before dropout) are saved for the backward, both or
 * neither (NULL for inference). */
int pxr_lightsans_fwd_f32(const float* qkv, const float* theta, const float* A, int B, int L, int D, int H, int K, float p_drop,
                          uint64_t seed, uint32_t stream_id, const int64_t* step_dev, float* ctx, float* pi, float* probs, float* KVp,
                          void* stream);
/* Its backward from dctx [B*L, D]: dqkv [B*L, 3D] (every path into k and v summed: pooled, through the interest logits and, for v,
 * the positional one); dKVp [B, 2K, D] = d Kp | d Vp; per-sequence parts dtheta_part [B, 2 D K] of d thK | d thV and dA_part
 * [B, H L L] of d A, each reduced over B by pxr_colsum_f32.  Same dropout arguments as the forward. */
int pxr_lightsans_bwd_f32(const float* dctx, const float* qkv, const float* theta, const float* A, const float* pi, const float* probs,
                          const float* KVp, int B, int L, int D, int H, int K, float p_drop, uint64_t seed, uint32_t stream_id,
                          const int64_t* step_dev, float* dqkv, float* dKVp, float* dtheta_part, float* dA_part, void* stream);
/* Position probabilities (layers.py:862-868), one workgroup per head: pqk [L, 2D] = pos_ln(P) Wpq^T + bpq | pos_ln(P) Wpk^T + bpk;
 * A[h, i, j] = softmax over the queries i of (pq_h[i] . pk_h[j]) (2 dh)^-1/2 / sqrt(dh).  The backward takes dA [H, L, L] (the
 * reduced dA_part) to dpqk [L, 2D] = d pq | d pk. */
int pxr_lightsans_pos_fwd_f32(const float* pqk, int L, int D, int H, float* A, void* stream);
int pxr_lightsans_pos_bwd_f32(const float* pqk, const float* A, const float* dA, int L, int D, int H, float* dpqk, void* stream);

/* ---- ids to rows of a table that holds several embeddings (csrc/rows.hip) --------------------------------------------------- */
/* MF, VBPR, ACF, DIN and the pooled pair models keep their embeddings in ONE table buffer whose row 0 is a spare (the sparse-row
 * kernels treat id 0 as padding / an empty slot).  A step's occurrences are 1 .. 4 segments of ids laid end to end: occurrence o of
 * a segment reads rows[o] = base + id; gidx[o] (may be NULL) = the row its gradient is summed into: rows[o], or 0 (dropped by
 * pxr_embed_grad_rows_f32) for id 0 of a segment with pad0 set.  An id outside [0, n) ORs bit 0 into the status word (clamped).
 * A segment with count 0 may have ids == NULL; every base + n < 2^40; 0 < the sum of the counts < 2^31.  The descriptors are host
 * memory, read during the call only.  The models' segment lists (U users, I items):
 *   MF    [1 + U + I, D]       user -> 1 + u | item.view(-1) -> 1 + U + i            (item [B, 2] = (positive, negative))
 *   VBPR  [1 + U + I + U, Dh]  user -> 1 + u | user -> 1 + U + I + u | item.view(-1) -> 1 + U + i
 *   ACF   [1 + I + U, E]       profile -> 1 + i (pad0) | items -> 1 + i (pad0) | user -> 1 + I + u
 *   DIN / pooled pair models [1 + I, D]: ACF's list without the user segment
 * (evaluation passes the user segments alone). */
typedef struct pxr_row_segment {
  const int64_t* ids;
  int64_t count, n, base;
  int32_t pad0, reserved;
} pxr_row_segment;
/* segments: n_segments pxr_row_segment */
int pxr_table_rows_i64(const void* segments, int n_segments, int64_t* rows, int64_t* gidx, void* stream);

/* ---- MF (model/IDNet/mf.py, layers.py:239-294 MLPLayers; csrc/mf.hip) ------------------------------------------------------- */
/* The table is ONE [1 + n_users + n_items, D] buffer: user u at row 1 + u, item i at row 1 + n_users + i, row 0 a spare.
 * rows[3B] (pxr_table_rows_i64) = [1 + user[b] for b < B | the rows of item.view(-1)]. */
/* Pair loss head (mf.py forward): x_b = <u_b, i+_b> - <u_b, i-_b>, lossrow[b] = -(1e-8 + log sigmoid(x_b)), loss = mean,
 * coef[b] = d loss / d x_b = -(1 - sigmoid(x_b)) / B.  rows != NULL: u_b = ufeat[rows[b]], i+-_b = ifeat[rows[B + 2b (+1)]]
 * (the table, ufeat == ifeat); rows == NULL: the tower outputs, u_b = ufeat[b] ([B, H]), i+-_b = ifeat[2b (+1)] ([2B, H]).
 * H % 4 == 0, H <= 4096. */
int pxr_mf_pair_fwd_f32(const float* ufeat, const float* ifeat, const int64_t* rows, int H, int B, float* coef, float* lossrow,
                        float* loss, void* stream);
/* The same head with the shift as an argument: lossrow[b] = -(eps + log sigmoid(x_b)), coef unchanged; pxr_mf_pair_fwd_f32 is this
 * entry with eps = 1e-8f, bit for bit.  eps = 0 is momf.py:59's loss, -mean log sigmoid(x_b).  ufeat and ifeat are indexed through
 * the one rows[3B] list with two base pointers, so ufeat = MOMF's user table [1 + n_users, H], ifeat = the encoder's output
 * E [M, H] and rows = [1 + user | idx.view(-1)] is MOMF's forward without a gather.  log sigmoid(x) is computed as min(x, 0) -
 * log1p(exp(-|x|)) and stays finite for every finite x (about x for x << 0); the reference's log(sigmoid(x)) is -inf in float32
 * once sigmoid(x) underflows (x below about -103.97), where the two differ by design.  eps finite and >= 0. */
int pxr_mf_pair_fwd_eps_f32(const float* ufeat, const float* ifeat, const int64_t* rows, int H, int B, float eps, float* coef,
                            float* lossrow, float* loss, void* stream);
/* Its backward onto the tower outputs: du[b] = c_b (i+_b - i-_b), di[2b] = c_b u_b, di[2b + 1] = -c_b u_b with c_b = coef[b] *
 * grad_scale * (*grad_scale_dev if given). */
int pxr_mf_pair_bwd_f32(const float* ufeat, const float* ifeat, const float* coef, int H, int B, float grad_scale,
                        const float* grad_scale_dev, float* du, float* di, void* stream);
/* The step's table gradient as sparse rows (SparseRows: sp_idx int64 [cap], sp_rows [cap, D], *sp_n = 3B): slot o of occurrence
 * o = (rows[o], the sum of every occurrence of that row in ascending order) for the first occurrence of a row, (0, zeros) for the
 * others.  occ != NULL: occurrence k contributes occ[k, :] ([3B, D], the towers' input gradients in the rows[] layout); occ ==
 * NULL: the head's formula on table [n_table, D] with coef (scaled as above).  O(B D) work, deterministic, no atomics.  D % 4 ==
 * 0, D <= 4096, cap >= 3B. */
int pxr_mf_table_grad_f32(const float* table, int64_t n_table, int D, const int64_t* rows, int B, const float* coef,
                          const float* occ, float grad_scale, const float* grad_scale_dev, int64_t* sp_idx, float* sp_rows,
                          int32_t* sp_n, int64_t cap, void* stream);
/* MOMF (model/PixelNet/momf.py): the same per-occurrence sums over TWO row spaces and into two sinks, one launch.  rows[3B] = [1 +
 * user[b] for b < B | idx.view(-1)]: rows of utable [n_utable, D] (row 0 a spare), then positions into E [M, D] (base 0: there is
 * no padding position).  Both already checked and clamped (pxr_table_rows_i64).
 *   user sink (sparse, *sp_n = B): slot o < B = (rows[o], sum_b c_b (E[p_b] - E[n_b]) over the samples b of that user, ascending) at
 *     the first occurrence of the row, (0, zeros) at the others -- pxr_mf_table_grad_f32's user slots, bit for bit;
 *   item sink (dense): dE [M, D] is zeroed by this entry, then dE[m, :] = the sum over the occurrences of position m in ascending
 *     order of +-c_b u_b, stored by the first occurrence; a row nobody reads is +0.0 whatever dE held.
 * occ != NULL (towers): occurrence k contributes occ[k, :] ([3B, D]) to either sink and utable, E, coef may be NULL; occ == NULL:
 * the head's formula, c_b = coef[b] * grad_scale * (*grad_scale_dev if given).  O(B D) work, vector stores only, no atomics, the
 * same bits from run to run.  D % 4 == 0, D <= 4096, cap >= B; dE must not alias an operand. */
int pxr_momf_pair_grad_f32(const float* utable, int64_t n_utable, const float* E, int64_t M, int D, const int64_t* rows, int B,
                           const float* coef, const float* occ, float grad_scale, const float* grad_scale_dev, int64_t* sp_idx,
                           float* sp_rows, int32_t* sp_n, int64_t cap, float* dE, void* stream);
/* BatchNorm1d (training) + tanh over x [R, H]: batch mean and biased variance (eps), y = tanh(gamma xhat + beta); mean / rstd
 * [H] saved for the backward; running_mean / running_var updated with momentum and the unbiased variance, *num_batches_tracked
 * += 1 (may be NULL).  Column sums in a fixed order.  R >= 2, H % 4 == 0, H <= 4096; y must not alias x. */
int pxr_mf_bn_tanh_fwd_f32(const float* x, int R, int H, const float* gamma, const float* beta, float eps, float momentum,
                           float* running_mean, float* running_var, int64_t* num_batches_tracked, float* y, float* mean,
                           float* rstd, void* stream);
/* Its backward from dy [R, H] through the tanh (y) and the batch statistics: dx [R, H], dgamma / dbeta [H] (overwritten). */
int pxr_mf_bn_tanh_bwd_f32(const float* dy, const float* x, const float* y, const float* mean, const float* rstd,
                           const float* gamma, int R, int H, float* dx, float* dgamma, float* dbeta, void* stream);
/* Eval form: y = tanh(gamma (x - running_mean) / sqrt(running_var + eps) + beta), elementwise over [R, H]. */
int pxr_mf_bn_tanh_eval_f32(const float* x, int64_t R, int H, const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, float eps, float* y, void* stream);

/* ---- VBPR (model/ViNet/vbpr.py; csrc/vbpr.hip) ----------------------------------------------------------------------------- */
/* The tables are ONE [1 + 2 n_users + n_items, Dh] buffer in the reference's parameter order: user_id_embedding row u at 1 + u,
 * item_id_embedding row i at 1 + n_users + i, user_modal_embedding row u at 1 + n_users + n_items + u, row 0 a spare.  rows[4B]
 * (pxr_table_rows_i64) = [id row of user[b] | modal row of user[b] | id rows of item.view(-1)]; the 2B user rows alone in
 * evaluation (vbpr.py:57-60 forward's three embedding lookups, :79-82 predict's). */
/* Feature gather with the visual bias fused (vbpr.py:61,65 self.v_feat[item] read twice, :94 compute_item_all's bias): out[r, :]
 * = feat[item[r], :] ([n, F], the projection GEMM's operand) and beta[r] = <feat[item[r], :], wb> from one read of the row.
 * item == NULL: row r itself (n <= n_items); out == NULL: beta only.  Item ids outside [0, n_items) flag and clamp.  F % 4 == 0. */
int pxr_vbpr_gather_f32(const float* feat, int64_t n_items, int F, const int64_t* item, int64_t n, const float* wb, float* out,
                        float* beta, void* stream);
/* Pair head (vbpr.py:64-70): s_{b,t} = <uid_b, iid_{b,t}> + <um_b, e[2b + t]> + beta[2b + t] with the id rows read from table at
 * rows[4B]; x_b = s_{b,0} - s_{b,1}; lossrow[b] = -log(1e-8 + sigmoid(x_b)), loss = mean; coef[b] = d loss / d x_b.
 * Dh % 4 == 0, Dh <= 4096. */
int pxr_vbpr_pair_fwd_f32(const float* table, const int64_t* rows, const float* e, const float* beta, int Dh, int B, float* coef,
                          float* lossrow, float* loss, void* stream);
/* Its backward (autograd of vbpr.py:57-70), c_b = coef[b] * grad_scale * (*grad_scale_dev if given): de[2b + t] = +-c_b um_b
 * ([2B, Dh], the weight-gradient GEMM's operand), csign[2b + t] = +-c_b, and the three tables' gradient as sparse rows
 * (SparseRows: sp_idx int64 [cap], sp_rows [cap, Dh], *sp_n = 4B): slot o of occurrence o = (rows[o], the sum of every occurrence
 * of that row in ascending order) for the first occurrence of a row, (0, zeros) for the others; occurrences contribute c_b (iid+ -
 * iid-) (id row of the user), c_b (e+ - e-) (modal row), +-c_b uid_b (item rows).  Deterministic, no atomics.  cap >= 4B. */
int pxr_vbpr_pair_bwd_f32(const float* table, const int64_t* rows, const float* e, const float* coef, int Dh, int B,
                          float grad_scale, const float* grad_scale_dev, float* de, float* csign, int64_t* sp_idx, float* sp_rows,
                          int32_t* sp_n, int64_t cap, void* stream);
/* Gradient of bias_projection.weight (autograd of vbpr.py:65): dwb[F] = sum_r csign[r] x[r, :] over the gathered rows x [R, F],
 * column sums in a fixed order.  F % 4 == 0. */
int pxr_vbpr_bias_grad_f32(const float* x, const float* csign, int R, int F, float* dwb, void* stream);
/* One side of the evaluation score as an inner product (vbpr.py:79-88 predict): out[r, :] = [a[ra, :] | b[rb, :] | s_r | 0 ...]
 * ([R, Dp]; ra = a_rows ? a_rows[r] : r, rb likewise, both operands Dh wide; s_r = s ? s[r] : 1).  Items: (item id rows,
 * projected features, visual bias); queries: (user id rows, user modal rows, 1).  Dh % 4 == 0, Dp % 4 == 0, Dp > 2 Dh. */
int pxr_vbpr_pack_f32(const float* a, const int64_t* a_rows, const float* b, const int64_t* b_rows, const float* s, int64_t R,
                      int Dh, int Dp, float* out, void* stream);

/* ---- CNN-F: conv2d by im2col, 2x2 max-pool (model/PixelNet/dvbpr.py:113-137; csrc/conv2d.hip) -------------------------------- */
/* A convolution is im2col over a chunk of images + the GEMMs above (y = col W^T + b with the ReLU epilogue, dW = dY^T col, dcol =
 * dY W) + col2im.  Padding 0, dilation 1: Ho = (H - kh) / sh + 1, Wo = (W - kw) / sw + 1.  An activation is addressed through its
 * four ELEMENT strides (n, c, h, w): the image is NCHW, a GEMM output [n Ho Wo, Cout] is NHWC.  Every offset is 64-bit; fp32; no
 * atomics.  Bad geometry (a kernel larger than the input, a non-positive stride, ldk not K rounded up to a multiple of 4) is an
 * error without a launch.
 * im2col (dvbpr.py:113-114,127 nn.Conv2d's unfold): col[(img, ho, wo), (c, i, j)] = x[img, c, ho sh + i, wo sw + j], K = C kh kw
 * columns in (c, i, j) order -- weight.view(Cout, K) is the GEMM's B operand as it stands -- in rows of ldk floats; columns
 * [K, ldk) are written +0.0.  col 16-byte aligned. */
int pxr_conv2d_im2col_f32(const float* x, int64_t x_sn, int64_t x_sc, int64_t x_sh, int64_t x_sw, int64_t n, int C, int H, int W,
                          int kh, int kw, int sh, int sw, float* col, int64_t ldk, void* stream);
/* col2im, the data gradient in gather form (autograd of dvbpr.py:127): dx[img, c, h, w] = the sum of the at most kh kw entries of
 * dcol that im2col filled from that element, kh outer, kw inner; +0.0 where no window covers it (a stride remainder).  dx is
 * addressed through its strides and written whole. */
int pxr_conv2d_col2im_f32(const float* dcol, int64_t ldk, int64_t n, int C, int H, int W, int kh, int kw, int sh, int sw, float* dx,
                          int64_t d_sn, int64_t d_sc, int64_t d_sh, int64_t d_sw, void* stream);
/* nn.MaxPool2d(2) (dvbpr.py:117,129): p[img, c, hp, wp] = max of the 2x2 window, Hp = H / 2, Wp = W / 2 (floor: a trailing odd row /
 * column is dropped).  Both sides through strides (the last pool writes (c, h, w) order for fcs.0).  H, W >= 2. */
int pxr_maxpool2x2_fwd_f32(const float* y, int64_t y_sn, int64_t y_sc, int64_t y_sh, int64_t y_sw, int64_t n, int C, int H, int W,
                           float* p, int64_t p_sn, int64_t p_sc, int64_t p_sh, int64_t p_sw, void* stream);
/* Its backward fused with the mask of the ReLU in front of it (autograd of dvbpr.py:127-129): y = the ReLU'd conv output that was
 * pooled; dy[pix] = dp[window of pix] where pix is the FIRST maximum of its window in row-major order (torch's rule) and y[pix] >
 * 0, else +0.0; dropped rows / columns get +0.0.  dy has y's strides and is written whole. */
int pxr_maxpool2x2_relu_bwd_f32(const float* y, int64_t y_sn, int64_t y_sc, int64_t y_sh, int64_t y_sw, const float* dp, int64_t p_sn,
                                int64_t p_sc, int64_t p_sh, int64_t p_sw, int64_t n, int C, int H, int W, float* dy, void* stream);

/* ---- DVBPR (model/PixelNet/dvbpr.py; csrc/dvbpr.hip) ----------------------------------------------------------------------- */
/* The tables are ONE [1 + 2 n_users + n_items, Dh] buffer in the reference's registration order: theta_users row u at 1 + u,
 * gamma_users row u at 1 + n_users + u, gamma_items row i at 1 + 2 n_users + i, row 0 a spare.  rows[6B] (pxr_table_rows_i64) =
 * [gamma row of user[b] | theta row of user[b] | gamma rows of item_id.view(-1) | positions index.view(-1) into E, base 0]; E
 * [M, Dh] = the encoder's output, one row per distinct image of the batch.
 * Pair head (dvbpr.py:49-62): x_b = <gu_b, gi+ - gi-> + <tu_b, E[p_b] - E[n_b]>; lossrow[b] = -log sigmoid(x_b) (no 1e-8), loss =
 * mean, coef[b] = d loss / d x_b.  Dh % 4 == 0, Dh <= 4096. */
int pxr_dvbpr_pair_fwd_f32(const float* table, const int64_t* rows, const float* E, int Dh, int B, float* coef, float* lossrow,
                           float* loss, void* stream);
/* Its backward (autograd of dvbpr.py:49-62), c_b = coef[b] * grad_scale * (*grad_scale_dev if given): the three tables' gradient as
 * sparse rows (slots as pxr_vbpr_pair_bwd_f32; *sp_n = 4B; contributions c_b (gi+ - gi-), c_b (E[p] - E[n]), +-c_b gu_b) and dE
 * [M, Dh] dense: dE[m] = the sum over the positions k with index.view(-1)[k] == m, ascending, of +-c_b tu_b; +0.0 for a row no
 * position names.  Position 0 is a real image.  Deterministic, no atomics.  cap >= 4B. */
int pxr_dvbpr_pair_bwd_f32(const float* table, const int64_t* rows, const float* E, int64_t M, const float* coef, int Dh, int B,
                           float grad_scale, const float* grad_scale_dev, float* dE, int64_t* sp_idx, float* sp_rows, int32_t* sp_n,
                           int64_t cap, void* stream);

/* ---- ACF (model/ViNet/acf.py; csrc/acf.hip) ------------------------------------------------------------------------------- */
/* The tables are ONE [1 + n_items + n_users, E] buffer in the reference's parameter order: item_model row i at 1 + i (item 0 is
 * the reference's padding row: read, decayed, never given a gradient), user_embedding row u at 1 + n_items + u, row 0 a spare.
 * Occurrences (pxr_table_rows_i64) in the order [profile ids | item ids (positive, negative per sample) | user ids], gidx 0 for
 * item id 0. */
/* Region attention (acf.py ACFFeatureNet.forward after the two Linears), r = b P + p: s_h = <w, relu(xt[r, h, :] + ut[b, :])>,
 * beta[r, :] = softmax_H(s), pooled[r, :] = sum_h beta[r, h] x[r, h, :]; a masked r (profile[r] == 0) gets beta = 0 and pooled =
 * 0.  x, xt [B P, H, E]; ut [B, E]; w [E] (feats.w.weight; its scalar bias cancels in the softmax).  One pass over x and xt,
 * fixed summation order.  H <= 1024, E % 4 == 0, E <= 4096. */
int pxr_acf_region_fwd_f32(const float* x, const float* xt, const float* ut, const float* w, const int64_t* profile, int B, int P,
                           int H, int E, float* beta, float* pooled, void* stream);
/* Its backward from dpooled [B P, E]: dxt [B P, H, E] (gradient of xt = of relu's argument), dut [B, E] = sum over the user's P H
 * positions of dxt in ascending (p, h), dw_part [B P, E] whose column sum is d w (pxr_colsum_f32).  ws: B P E floats.  The
 * gradient of x is NOT written here: see pxr_acf_region_dx_f32.  dxt must not alias x or xt. */
int pxr_acf_region_bwd_f32(const float* dpooled, const float* x, const float* xt, const float* ut, const float* w,
                           const int64_t* profile, const float* beta, int B, int P, int H, int E, float* dxt, float* dut,
                           float* dw_part, float* ws, void* stream);
/* Gradient of dim_reductor's pre-activation, in place: dx [R, H, E] holds the feats.w_x input gradient (dxt W) on entry and
 * (dx + beta[r, h] dpooled[r, :]) (x > 0) on exit -- the pooled path added and the ReLU applied in one pass. */
int pxr_acf_region_dx_f32(float* dx, const float* x, const float* beta, const float* dpooled, int64_t R, int H, int E,
                          void* stream);
/* Item attention and the user vector (acf.py ACFUserNet.forward after its three Linears): t_p = <w, relu(uw[b, :] + pq[r, :] +
 * cx[r, :])>, alpha[b, :] = softmax_P(t) over the p with profile[r] != 0 (0 elsewhere; all zero for an empty profile),
 * user[b, :] = uw[b, :] + sum_p alpha[b, p] prof[r, :].  uw [B, E]; pq, cx, prof [B P, E]; w [E].  P <= 1024. */
int pxr_acf_item_fwd_f32(const float* uw, const float* pq, const float* cx, const float* prof, const float* w,
                         const int64_t* profile, int B, int P, int E, float* alpha, float* user, void* stream);
/* Its backward from duser [B, E]: da [B P, E] (the gradient of pq and of cx alike), dprof [B P, E] = alpha duser (the direct path
 * onto the profile rows), duw [B, E] = duser + sum_p da, dw_part [B, E] whose column sum is d w.  Outputs must not alias inputs. */
int pxr_acf_item_bwd_f32(const float* duser, const float* uw, const float* pq, const float* cx, const float* prof, const float* w,
                         const float* alpha, int B, int P, int E, float* da, float* dprof, float* duw, float* dw_part,
                         void* stream);

/* ---- VISRANK (model/ViNet/visrank.py; csrc/visrank.hip) -------------------------------------------------------------------- */
/* unit[i, :] = feat[i, :] / max(||feat[i, :]||_2, eps) ([N, F], F % 4 == 0): the operand of the cosine scoring, made once per
 * model (visrank.py:44 torch.cosine_similarity, eps 1e-8). */
int pxr_visrank_unit_rows_f32(const float* feat, int64_t N, int F, float eps, float* unit, void* stream);
/* Workspace of the call below in bytes; -1 outside its limits (B >= 1, 1 <= H <= 64, N >= 1, 1 <= K <= 32).  Grows with B, K and
 * the number of item splits only. */
int64_t pxr_visrank_topk_ws_bytes(int B, int H, int N, int K);
/* Fused VISRANK scoring (visrank.py:37-56 predict + trainer.py:333-336 masks + collector's torch.topk): per user b with the window
 * w = the nonzero tail of window[b, :] (int64 [B, H], left-padded with 0, h = len(w) >= 1), S[r, j] = <unit[w[r]], unit[j]>,
 * score[j] = the mean of the min(top_k, h) largest of S[:, j] (top_k in 1..16; top_k == 0: the mean of all h), score[0] = -inf and
 * score[i] = -inf for every i in hist_items[hist_ptr[b] .. hist_ptr[b + 1]) (the CSR of pxr_score_topk_f32; may be NULL);
 * topk_idx int64 / topk_val [B, K] = the K best, descending (fewer than K unmasked items: id -1, value -inf).  S never reaches
 * memory.  A window or history id outside [0, N), a 0 inside the window's tail or an empty window ORs bit 0 into the status word
 * and leaves both outputs untouched.  F % 4 == 0, N * F * 4 < 2 GiB. */
int pxr_visrank_topk_f32(const float* unit, int N, int F, const int64_t* window, int B, int H, int top_k, const int32_t* hist_ptr,
                         const int64_t* hist_items, int K, int64_t* topk_idx, float* topk_val, void* ws, int64_t ws_bytes,
                         void* stream);

/* ---- CuratorNet (model/ViNet/curatornet.py; csrc/curator.hip) ------------------------------------------------------------- */
/* Profile pooling (curatornet.py:77-79 forward, :96-99 predict: AdaptiveMaxPool2d / AdaptiveAvgPool2d((1, E)) on [B, L, E], then
 * torch.cat): cat[b, :] = [max over l | mean over l] over ALL L positions, padding included (the mean divides by L); argmax uint8
 * [B, E] (may be NULL) = the position of the max, the FIRST among equal values.  ids == NULL: h is [B, L, E] (n_items unused);
 * ids int64 [B, L]: h is the item matrix [n_items, E] and position (b, l) reads row ids[b, l] (predict's item_feature[user]) --
 * an id outside [0, n_items) ORs bit 0 into the status word and is clamped.  E % 4 == 0, E <= 4096, 1 <= L <= 255. */
int pxr_curator_pool_f32(const float* h, const int64_t* ids, int64_t n_items, int B, int L, int E, float* cat, uint8_t* argmax,
                         void* stream);
/* Its backward joined with the head's item gradient and the SELU of selu_common2 (autograd of curatornet.py:67-79): dpre
 * [B (L + 2), E], rows [B L profile | 2B positive, negative]: profile row (b, l) = (dcat[b, E + e] / L + [l == argmax[b, e]]
 * dcat[b, e]) * dact[row, e]; row B L + j = di[j, e] * dact[row, e].  dcat [B, 2E], di [2B, E] (pxr_mf_pair_bwd_f32), dact
 * [B (L + 2), E] = selu' saved by the forward.  Every element written once: no atomics. */
int pxr_curator_pool_bwd_f32(const float* dcat, const uint8_t* argmax, const float* di, const float* dact, int B, int L, int E,
                             float* dpre, void* stream);
/* Pair head on the towers' outputs (curatornet.py:86-88): x_b = <u_b, i+_b> - <u_b, i-_b> with ufeat [B, H], ifeat [2B, H] =
 * (positive, negative) per sample; lossrow[b] = -log(1e-8 + sigmoid(x_b)) -- the 1e-8 INSIDE the log, unlike mf.py's head --
 * loss = mean, coef[b] = d loss / d x_b = -(1/B) sigmoid(x)(1 - sigmoid(x)) / (1e-8 + sigmoid(x)).  The backward is
 * pxr_mf_pair_bwd_f32 on this coef.  H % 4 == 0, H <= 4096. */
int pxr_curator_pair_fwd_f32(const float* ufeat, const float* ifeat, int H, int B, float* coef, float* lossrow, float* loss,
                             void* stream);
/* out = a * b elementwise (n % 4 == 0; out may alias a or b): the head's user gradient times selu' of selu_pu3 -- autograd of
 * F.selu at curatornet.py:82, the one activation of the step with no GEMM in front of it whose epilogue could multiply. */
int pxr_mul_f32(const float* a, const float* b, float* out, int64_t n, void* stream);

/* ---- DIN (model/IDNet/din.py with SequenceAttLayer, model/layers.py:460-514; csrc/din.hip) --------------------------------- */
/* Occurrences of a batch: o in [0, B L) = history position (b, l); o = B L + 2 b + c = candidate c of sample b (0 positive, 1
 * negative).  Pair rows of the attention MLP: r = (c B + b) L + l.  rows int64 [B L + 2 B] = the table row every occurrence reads
 * (already range-checked: pxr_table_rows_i64, DIN's segments).
 * Attention input (din.py:59-62 item_embedding(items); layers.py:486-491 repeat / cat): emb[o, :] = table[rows[o], :] and
 * x[r, :] = [q | k | q - k | q * k] with q = the candidate's row, k = the history row.  emb [B L + 2 B, D], x [2 B L, 4 D].
 * D % 4 == 0, D <= 4096. */
int pxr_din_att_input_f32(const float* table, const int64_t* rows, int B, int L, int D, float* emb, float* x, void* stream);
/* Head forward (layers.py:493-512 dense / masked_fill / divide / matmul; din.py:53 the score; din.py:79-81 the loss): alast
 * [2 B L, hl] = the last hidden layer's activations, wd [hl], bd [1] = attention.dense, profile int64 [B, L] (0 = padding).
 * s[r] = 0 at padding, else (<alast[r], wd> + bd) / sqrt(D); kq[r] = <k_l, q_c>; score_c = sum_l s kq in ascending l;
 * head [2 + 3 B] = loss | 0.01 / (B ||emb||_2) (0 when the norm is 0) | coef [B] = d loss / d (score_0 - score_1) | the score
 * differences [B] | per-sample sums of squares [B].  loss = -mean log(sigmoid(x) + 1e-8) + 0.01 ||emb||_2 / B, the norm over all
 * B (L + 2) gathered rows (padding positions included), reduced in one fixed order. */
int pxr_din_head_fwd_f32(const float* alast, const float* wd, const float* bd, const float* emb, const int64_t* profile, int B,
                         int L, int D, int hl, float* s, float* kq, float* head, void* stream);
/* The same head with the regulariser's weight as an argument (PixelNet/modin.py:61: MODIN's loss is the first term alone, reg = 0;
 * IDNet/din.py:79: reg = 0.01, and the entry above is this one with that value, bit for bit): loss = -mean log(sigmoid(x) + 1e-8) +
 * reg ||emb||_2 / B and head[1] = reg / (B ||emb||_2), which is 0 when reg == 0 or the norm is 0 -- pxr_din_fold_bwd_f32 then adds an
 * exact zero.  The head layout does not depend on reg.  reg >= 0 and finite. */
int pxr_din_head_fwd_reg_f32(const float* alast, const float* wd, const float* bd, const float* emb, const int64_t* profile, int B,
                             int L, int D, int hl, float* s, float* kq, float* head, float reg, void* stream);
/* Head backward, first half (autograd of the above down to the last hidden layer): g = grad_scale * grad_scale_dev[0];
 * dsraw[r] = the gradient of dense's output (0 at padding), dz [2 B L, hl] = dsraw wd act' (dact = the derivative the forward
 * GEMM saved), dwd [hl] and dbd [1] = the gradients of attention.dense, summed over r in one fixed order. */
int pxr_din_head_bwd_f32(const float* alast, const float* dact, const float* wd, const int64_t* profile, const float* kq,
                         const float* head, int B, int L, int D, int hl, float grad_scale, const float* grad_scale_dev, float* dz,
                         float* dsraw, float* dwd, float* dbd, void* stream);
/* Head backward, second half: one gradient row per occurrence, occ [B L + 2 B, D].  With dx [2 B L, 4 D] = the MLP's input
 * gradient (blocks dx0 | dx1 | dx2 | dx3): candidate rows get g coef sum_l s k_l + sum_l (dx0 + dx2 + dx3 * k_l), history rows
 * sum_c (g coef s q_c + dx1 - dx2 + dx3 * q_c) -- autograd of din.py:53 and layers.py:491 -- and every row the regulariser's
 * g head[1] emb[o] (din.py:79).  A padding position's row is written as zeros (nn.Embedding(padding_idx=0) drops it). */
int pxr_din_fold_bwd_f32(const float* dx, const float* emb, const int64_t* profile, const float* s, const float* head, int B, int L,
                         int D, float grad_scale, const float* grad_scale_dev, float* occ, void* stream);
/* The first Linear of the attention MLP factorised over cat[q, k, q - k, q * k] (layers.py:491-492): W1 [h1, 4 D] ->
 * A = W1[:, 0:D] + W1[:, 2D:3D], Bm = W1[:, D:2D] - W1[:, 2D:3D], C = W1[:, 3D:4D], each [h1, D].  With the library's Linear on
 * the item table, A gives the once-per-evaluation term A q + b1 of pxr_din_topk_f32. */
int pxr_din_fold_w1_f32(const float* w1, int h1, int D, float* A, float* Bm, float* C, void* stream);
/* Workspace of the call below in bytes; -1 outside the fused limits (D % 4 == 0, 4 <= D <= 128, 1 <= h1 <= 128, 0 <= h2 <= 128,
 * 1 <= L <= 64, 1 <= K <= 32, N D 4 < 2 GiB).  Grows with B L h1 D (the scaled copies of C). */
int64_t pxr_din_topk_ws_bytes(int B, int L, int N, int D, int h1, int h2, int K);
/* Fused DIN evaluation (din.py:87-103 predict over CandiEvalDataset's [item_num, L + 1] id matrix per user + trainer.py:333-336
 * masks + the collector's torch.topk): per user b, window row l with window[b, l] != 0 and item n,
 *   z1 = aq[n, :] + Bm k_l + C (q_n * k_l),  s = dense(sigmoid(W2 sigmoid(z1) + b2)) / sqrt(D)   (h2 == 0: dense(sigmoid(z1))),
 *   score[b, n] = sum_l s <k_l, q_n>     (a padded row contributes exactly 0; an all-padding window scores 0 everywhere)
 * with aq [N, h1] = A q_n + b1, bm / cm [h1, D] from pxr_din_fold_w1_f32, w2 [h2, h1], b2 [h2], wd [h_last], bd [1].
 * score[b, 0] = -inf and score[b, i] = -inf for i in hist_items[hist_ptr[b] .. hist_ptr[b + 1]) (the CSR of pxr_score_topk_f32;
 * may be NULL); topk_idx int64 / topk_val [B, K] = the K best, descending (fewer than K unmasked items: id -1, value -inf).  No
 * [B, L, N, *] value reaches memory.  A window or history id outside [0, N) ORs bit 0 into the status word and leaves both outputs
 * untouched; nothing is read out of range. */
int pxr_din_topk_f32(const float* table, int N, int D, const int64_t* window, int B, int L, const float* aq, const float* bm,
                     const float* cm, int h1, const float* w2, const float* b2, int h2, const float* wd, const float* bd,
                     const int32_t* hist_ptr, const int64_t* hist_items, int K, int64_t* topk_idx, float* topk_val, void* ws,
                     int64_t ws_bytes, void* stream);

/* ---- DSSM and FM (model/IDNet/dssm.py, fm.py; csrc/pool.hip, MODE_POOL of csrc/embed_grad.hip) ------------------------------ */
/* Occurrences of a batch, as for DIN: o in [0, B L) = history position (b, l); o = B L + 2 b + c = target c of sample b (0
 * positive, 1 negative).  rows int64 [B L + 2 B] = the row of `table` [n_table, D] every occurrence reads; a history entry equal
 * to pad_row is "no item" (training: pxr_table_rows_i64's rows over the [1 + I, D] table, pad_row 1; evaluation windows over an item
 * matrix: the ids themselves, pad_row 0).  Any other entry outside [0, n_table) ORs bit 0 into the status word and is clamped;
 * nothing is read out of range.  Limits of all four: D % 4 == 0, 0 < D <= 4096, L >= 1, B (L + 2) < 2^30; table, U, G and
 * uniq_rows 16-byte aligned.  One fixed summation order (l ascending), no float atomics: bit-identical from run to run.
 *
 * Masked pooling (dssm.py:46-55 avg_emb, fm.py:47-55 mask_emb + the sum): U[b, :] = sum over the real positions of
 * table[rows[b, l], :]; mean != 0 divides by (cnt + 1e-8f), cnt the number of real positions -- an fp32 division (torch.div); an
 * empty profile gives exactly 0.  w[b] = the factor the backward multiplies a history occurrence's gradient by: 1 / (cnt + 1e-8f)
 * (mean) or 1 (sum), and 0 for an empty profile.  rows [B, L] (only the B L history entries are read), U [B, D], w [B]. */
int pxr_pool_rows_f32(const float* table, int64_t n_table, int D, const int64_t* rows, int64_t pad_row, int B, int L, int mean,
                      float* U, float* w, void* stream);
/* The step without an MLP in one launch: the pooling above (same arithmetic: U and w are bit-identical to pxr_pool_rows_f32's),
 * x_b = <U_b, table[p_b]> - <U_b, table[n_b]> over the target rows rows[B L + 2 b + {0, 1}], lossrow[b] = -log(1e-8 + sigmoid(x_b))
 * (the 1e-8 INSIDE the log: dssm.py:68, fm.py:66), coef[b] = d loss / d x_b, loss = the mean of lossrow in
 * pxr_mf_pair_fwd_f32's reduction order.  rows [B L + 2 B]; U [B, D]; w, coef, lossrow [B]; loss [1].  No output may alias the
 * table. */
int pxr_pool_pair_fwd_f32(const float* table, int64_t n_table, int D, const int64_t* rows, int64_t pad_row, int B, int L, int mean,
                          float* U, float* w, float* coef, float* lossrow, float* loss, void* stream);
/* Its backward as the COMPACT gradient block G [3 B, D]: with c_b = coef[b] * grad_scale * (grad_scale_dev ? *grad_scale_dev : 1),
 * G[b] = c_b (table[p_b] - table[n_b]) -- the gradient of U_b, ONE row for all L history occurrences of sample b --
 * G[B + 2 b] = c_b U_b and G[B + 2 b + 1] = -c_b U_b.  The pooling weight w[b] is NOT folded in: pxr_pool_table_grad_f32 applies
 * it.  U [B, D] as the forward wrote it; G must not alias U or the table. */
int pxr_pool_pair_bwd_f32(const float* table, int64_t n_table, int D, const int64_t* rows, int B, int L, const float* U,
                          const float* coef, float grad_scale, const float* grad_scale_dev, float* G, void* stream);
/* The table gradient in sparse form from the compact block, without one row per occurrence: gidx int64 [B L + 2 B] = the table row
 * every occurrence's gradient goes to (pxr_table_rows_i64's gidx: 0 at padding, dropped; ids outside [0, n_table) are dropped too).
 * Sorted as pxr_embed_grad_rows_f32 sorts its idx (same keys, same stable order), then summed in occurrence order with occurrence
 * o < B L reading w[o / L] * G[o / L, :] and occurrence o >= B L reading G[B + (o - B L), :].  What it writes equals
 * pxr_embed_grad_rows_f32 on the materialised [B (L + 2), D] rows up to the rounding of w * G (bit for bit where every w is 1).
 * uniq_idx / uniq_rows hold B (L + 2) entries / rows; ws: pxr_embed_grad_ws_bytes(B (L + 2)).  uniq_rows must not alias G. */
int pxr_pool_table_grad_f32(const int64_t* gidx, int B, int L, const float* G, const float* w, int D, int64_t n_table,
                            int64_t* uniq_idx, float* uniq_rows, int32_t* n_uniq_dev, void* ws, int64_t ws_bytes, void* stream);
/* The same gradient as a DENSE block over a batch-local row space (MODSSM / MOFM: the rows are the visual encoder's outputs for the
 * batch's distinct images, row 0 the zero image = "no item"): same inputs, same sort and the same segment sums in the same order,
 * written to d_rows[row, :] for every referenced row in (0, n_rows) -- bit for bit what pxr_pool_table_grad_f32 puts into
 * uniq_rows for that row.  Every other row of d_rows [n_rows, D] (row 0, unreferenced rows) is exactly +0.0 when the call returns,
 * whatever it held before: the entry zeroes the block itself.  Ids equal to 0 or outside [0, n_rows) are dropped.  No float
 * atomics, no [B (L + 2), D] buffer.  Limits: D % 4 == 0, 0 < D <= 4096, L >= 1, B (L + 2) < 2^30, 16-byte aligned G and d_rows;
 * ws: pxr_embed_grad_ws_bytes(B (L + 2)) (it also holds the unique-row list).  d_rows must not overlap G. */
int pxr_pool_dense_grad_f32(const int64_t* gidx, int B, int L, const float* G, const float* w, int D, int64_t n_rows, float* d_rows,
                            void* ws, int64_t ws_bytes, void* stream);
/* The dense sink for plain occurrence rows (PixelNet/modin.py:45-61 under autograd: DIN's backward leaves one gradient row per
 * occurrence, and the rows they belong to are visual_encoder outputs of the batch's distinct images): idx int64 [n] holds rows of an
 * [n_rows, D] matrix, rows [n, D] one gradient row per occurrence.  d_rows[row, :] for every referenced row in (0, n_rows) is bit
 * for bit what pxr_embed_grad_rows_f32 (scale 1) puts into uniq_rows for that id -- the same sort, the same segment sums in the
 * same order, another sink; every other row of d_rows [n_rows, D] (row 0, unreferenced rows) is exactly +0.0 when the call returns,
 * whatever it held before: the entry zeroes the block itself, on the same stream.  Ids equal to 0 or outside [0, n_rows) are
 * dropped.  No float atomics.  Limits: D % 4 == 0, 0 < D <= 4096, 0 < n < 2^30, 16-byte aligned rows and d_rows;
 * ws: pxr_embed_grad_ws_bytes(n) (it also holds the unique-row list and its count).  d_rows must not overlap rows. */
int pxr_embed_grad_dense_f32(const int64_t* idx, int64_t n, const float* rows, int D, int64_t n_rows, float* d_rows, void* ws,
                             int64_t ws_bytes, void* stream);
/* The dense sink for the sequence models' three-term table gradient (PixelNet/mobert4rec.py under autograd, each distinct image
 * encoded once: the "table" is E [n_rows, D] = visual_encoder(images), items holds positions into it).  items, B, L and the layout
 * (id_bstride, in_off, pos_off, neg_off) are pxr_seq_occ_sort's; dx0 [B L, D], out [B L, D], coef [B L] are pxr_sasrec_occ_segsum's.
 * d_rows[row, :] for every referenced row in (0, n_rows) is bit for bit what pxr_seq_occ_sort + pxr_sasrec_occ_segsum (scale 1)
 * leave in uniq_rows for that id -- the same keys, the same sort, the same segment sums in the same order, another sink; every
 * other row of d_rows [n_rows, D] (row 0, unreferenced rows) is exactly +0.0 when the call returns, whatever it held before: the
 * entry zeroes the block itself, on the same stream.  Key 0 and ids outside [0, n_rows) are dropped; the latter also set the
 * bad-index bit of the status word.  No float atomics.  Limits: D % 4 == 0, 0 < D <= 4096, 3 B L < 2^30, 16-byte aligned dx0, out
 * and d_rows; ws: pxr_embed_grad_ws_bytes(3 B L) (it also holds the unique-row list and its count).  d_rows must not overlap dx0
 * or out. */
int pxr_seq_occ_dense_f32(const int64_t* items, int B, int L, int64_t id_bstride, int64_t in_off, int64_t pos_off, int64_t neg_off,
                          const float* dx0, const float* out, const float* coef, int D, int64_t n_rows, float* d_rows, void* ws,
                          int64_t ws_bytes, void* stream);

/* ---- WideDeep (model/IDNet/widedeep.py with MLPLayers, model/layers.py:239-281; csrc/widedeep.hip) ------------------------- */
/* Rows of every [2 B, *] operand: r = 2 b + c, c = 0 the plane [profile_b | positive], c = 1 the plane [profile_b | negative]
 * (widedeep.py:55 view(batch_size * 2, -1)).  The first Linear W1 [h1, (L + 1) D] splits over the concatenation into the history
 * block W1[:, :L D] and the target block W1[:, L D:]; the two planes of a sample share the history, so its product is made once.
 * Join (widedeep.py:56, the first Dropout(0) / Linear / ReLU of MLPLayers): zh [B, h1] = Xh W1[:, :L D]^T, zt [2 B, h1] =
 * Xt W1[:, L D:]^T (library GEMMs) -> a1[r, :] = relu(zh[r / 2] + zt[r] + b1), der = [a1 > 0] (what the backward multiplies by). */
int pxr_wd_join_f32(const float* zh, const float* zt, const float* b1, int B, int h1, float* a1, float* der, void* stream);
/* Its backward towards the shared history product: dzh[b, :] = dz1[2 b, :] + dz1[2 b + 1, :]   (autograd of widedeep.py:55-56). */
int pxr_wd_join_bwd_f32(const float* dz1, int B, int h1, float* dzh, void* stream);
/* Head forward (widedeep.py:53 the wide sum, :57 deep_predict_layer, :60-62 the loss) in the cancelled form: the history's wide
 * terms, wide_bias and the predict bias are the same in both planes of a sample, so
 *   x_b = <alast[2 b] - alast[2 b + 1], wp> + wide[p_b] - wide[n_b],   loss = -mean_b log(1e-8 + sigmoid(x_b)),
 * alast [2 B, hl] the last hidden layer's activations, wp [hl] = deep_predict_layer.weight, wide [n_items] =
 * wide_item_embedding.weight, target int64 [B, 2] = (p_b, n_b).  head [1 + 2 B] = loss | coef [B] = d loss / d x_b | x [B].  A
 * target outside [0, n_items) ORs bit 0 into the status word and is clamped.  One fixed reduction order. */
int pxr_wd_head_fwd_f32(const float* alast, const float* wp, const float* wide, int64_t n_items, const int64_t* target, int B,
                        int hl, float* head, void* stream);
/* Head backward (autograd of the above), g = grad_scale * grad_scale_dev[0]: dz [2 B, hl] = (c ? -g : g) coef_b wp act' (dact =
 * the derivative the forward saved), dwp [hl] = sum_b g coef_b (alast[2 b] - alast[2 b + 1]) in ascending b, dbp [1] and
 * dwide_bias [1] exactly 0 (both cancel in x_b), dwide [n_items] dense: zero except + g coef_b at p_b and - g coef_b at n_b, the
 * occurrences of one id summed in ascending 2 b + c; entry 0 (padding_idx) and flagged ids get nothing.  No float atomics. */
int pxr_wd_head_bwd_f32(const float* alast, const float* dact, const float* wp, const int64_t* target, int64_t n_items,
                        const float* head, int B, int hl, float grad_scale, const float* grad_scale_dev, float* dz, float* dwp,
                        float* dbp, float* dwide, float* dwide_bias, void* stream);
/* Workspace of the call below in bytes; -1 outside the fused limits (h1 % 4 == 0, 4 <= h1 <= 128, 0 <= h2 <= 128, 1 <= L <= 64,
 * 1 <= K <= 32).  Grows with B, K and the number of item splits only. */
int64_t pxr_wd_topk_ws_bytes(int B, int L, int N, int h1, int h2, int K);
/* Fused WideDeep evaluation (widedeep.py:66-79 predict over CandiEvalDataset's [item_num, L + 1] id matrix per user +
 * trainer.py:333-336 masks + the collector's torch.topk) on the factorised first Linear: T [N, h1] = deep W1[:, L D:]^T + b1,
 * hb [B, h1] = sum_l W1[:, l D:(l + 1) D] deep[window[b, l]] (padding reads row 0, like the reference), and per user
 *   s_b = sum_l wide[window[b, l]] + wide_bias + bp,
 *   score[b, n] = s_b + wide[n] + <wp, relu(W2 relu(T[n] + hb[b]) + b2)>      (h2 == 0: <wp, relu(T[n] + hb[b])>)
 * with w2 [h2, h1], b2 [h2], wp [h_last], wide [N], wide_bias / bp [1].  score[b, 0] = -inf and score[b, i] = -inf for i in
 * hist_items[hist_ptr[b] .. hist_ptr[b + 1]) (the CSR of pxr_score_topk_f32; may be NULL); topk_idx int64 / topk_val [B, K] = the
 * K best, descending (fewer than K unmasked items: id -1, value -inf).  No [B, N, *] value reaches memory.  A window or history
 * id outside [0, N) ORs bit 0 into the status word and leaves both outputs untouched; nothing is read out of range. */
int pxr_wd_topk_f32(const float* T, int N, int h1, const float* hb, const int64_t* window, int B, int L, const float* wide,
                    const float* wide_bias, const float* w2, const float* b2, int h2, const float* wp, const float* bp,
                    const int32_t* hist_ptr, const int64_t* hist_items, int K, int64_t* topk_idx, float* topk_val, void* ws,
                    int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PXR_H_ */
