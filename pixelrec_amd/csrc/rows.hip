// rows.hip -- ids to table rows for the models that keep several embeddings in ONE table buffer (MF, VBPR, ACF, DIN and the pooled
// pair models): a step's occurrences are up to four segments of ids laid end to end, and occurrence o of segment s reads table row
// base_s + id.  One thread per occurrence; an id outside [0, n_s) flags the status word and is clamped (checked_id).  Which segments
// a model has is the caller's (include/pxr.h: pxr_table_rows_i64; pixelrec_amd/ops.py builds the lists).
#include "pxr_common.h"
#include "../../include/pxr.h"   // pxr_row_segment

namespace pxr {

constexpr int ROWS_MAX_SEG = 4;
struct RowSegs {
  const int64_t* ids[ROWS_MAX_SEG];
  int64_t end[ROWS_MAX_SEG];      // one past the segment's last occurrence (unused segments: the total)
  int64_t n[ROWS_MAX_SEG], base[ROWS_MAX_SEG];
  int pad0[ROWS_MAX_SEG];
};

// rows[o] = the table row occurrence o reads; gidx[o] (optional) = the row its gradient goes to: 0 (none) for id 0 of a pad0 segment
__global__ void __launch_bounds__(256) table_rows_kernel(RowSegs a, int64_t* __restrict__ rows, int64_t* __restrict__ gidx,
                                                         int32_t* status) {
  const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= a.end[ROWS_MAX_SEG - 1]) return;
  const int64_t* ids = a.ids[0];
  int64_t start = 0, n = a.n[0], base = a.base[0];
  int pad0 = a.pad0[0];
#pragma unroll
  for (int s = 1; s < ROWS_MAX_SEG; ++s)       // (selects on constants: the argument arrays are never indexed by a register)
    if (o >= a.end[s - 1]) { ids = a.ids[s]; start = a.end[s - 1]; n = a.n[s]; base = a.base[s]; pad0 = a.pad0[s]; }
  const int64_t id = checked_id(ids[o - start], n, status, true);
  rows[o] = base + id;
  if (gidx) gidx[o] = (pad0 && id == 0) ? 0 : base + id;
}

}  // namespace pxr

using namespace pxr;

extern "C" int pxr_table_rows_i64(const void* segments, int n_segments, int64_t* rows, int64_t* gidx, void* stream) {
  PXR_REQUIRE(segments && rows, "pxr_table_rows_i64: null pointer");
  PXR_REQUIRE(n_segments >= 1 && n_segments <= ROWS_MAX_SEG, "pxr_table_rows_i64: need 1 .. %d segments (%d)", ROWS_MAX_SEG, n_segments);
  const pxr_row_segment* seg = (const pxr_row_segment*)segments;
  RowSegs a{};
  int64_t total = 0;
  for (int s = 0; s < ROWS_MAX_SEG; ++s) {
    if (s < n_segments) {
      PXR_REQUIRE(seg[s].count >= 0 && seg[s].count < (1ll << 31), "pxr_table_rows_i64: bad count of segment %d", s);
      PXR_REQUIRE(seg[s].count == 0 || seg[s].ids, "pxr_table_rows_i64: null id list with a positive count (segment %d)", s);
      PXR_REQUIRE(seg[s].n > 0 && seg[s].base >= 0 && seg[s].base + seg[s].n < (1ll << 40), "pxr_table_rows_i64: bad table size (segment %d)", s);
      a.ids[s] = seg[s].ids; a.n[s] = seg[s].n; a.base[s] = seg[s].base; a.pad0[s] = seg[s].pad0;
      total += seg[s].count;
    }
    a.end[s] = total;
  }
  PXR_REQUIRE(total > 0 && total < (1ll << 31), "pxr_table_rows_i64: need 0 < occurrences < 2^31 (%lld)", (long long)total);
  hipLaunchKernelGGL(table_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, rows, gidx,
                     pxr_status_word());
  return pxr_check_launch("pxr_table_rows_i64");
}
