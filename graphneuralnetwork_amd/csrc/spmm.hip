// spmm.hip -- GCN neighbour aggregation on gfx950: Y = A_hat . X (+ bias) over CSR.
//
// Replaces torch.spmm(adj, support) + bias at GCN/GCN.py:43-45 (reference
// Graph_conv_layer.forward). The reference reduces an uncoalesced fp32 COO with
// ATen's serial CPU kernel; here the adjacency is CSR (rowptr int64, col int32,
// val fp32) and rows are reduced by wavefronts according to the row-class plan
// of plan.hip:
//
//   * mid rows (1 < deg <= seg_len): one wavefront per row. The wave splits into
//     EPI = 64/LPR "edge slots" of LPR lanes; each slot gathers one neighbour row
//     per instruction with VW-wide (16 B for fp32x4) loads, so at F = 128 one wave
//     instruction moves two whole 512-B rows (1 KiB, the widest coalesced access
//     per instruction on CDNA4). The 64 (col, val) pairs of an edge chunk are
//     loaded coalesced once and broadcast to the slots with __shfl (ds_bpermute);
//     U slot loads are issued before the first FMA (U x 16 B per lane in flight).
//   * small rows (deg <= 1, 44% of the rows of the R-MAT graphs: self-loop only):
//     their (col, val) was resolved by the plan, so one wavefront packs
//     EPI x kSmallUnroll of them -- every slot gathers a different row -- instead
//     of spending a whole wave (and a rowptr -> col -> X dependency chain) per row.
//   * long rows (deg > seg_len, the power-law hubs): cut into seg_len-edge
//     segments, one wave each, written to a partial buffer and merged by a
//     fix-up workgroup per row (32 partial loads in flight, fixed order).
//   * slot partial sums are combined with xor-shuffles in a fixed order and no
//     float atomics are used anywhere: results are bitwise reproducible.
//   * the final Y rows are written with non-temporal stores (Y is not re-read by
//     this kernel; keeping it out of L2/MALL leaves room for hub rows of X:
//     +1-3 % measured, tools/spmm_ab.py).
// Segment waves are dispatched first (lowest block ids), then mid rows, then the
// packed small rows.
//
// The kernels are templates over the element type of the gathered table
// (spmm_kernels.hpp); this file holds their fp32 instantiations and entries, spmm_bf16.hip
// the ones that gather bf16 rows.
#include "spmm_kernels.hpp"

namespace gnn {

// err |= 1 for a task with no row, more than kTaskRows rows or rows outside [0, n_rows);
// err |= 2 for a task that overlaps the previous one (tasks must be disjoint and ascending)
__global__ __launch_bounds__(kBlock) void spmm_tasks_check_kernel(const int32_t* __restrict__ task_row,
                                                                  int64_t n_task, int64_t n_rows,
                                                                  int32_t* __restrict__ err) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= n_task) return;
  const int32_t rb = task_row[2 * t], re = task_row[2 * t + 1];
  int32_t e = 0;
  if (rb < 0 || re <= rb || re - rb > kTaskRows || re > n_rows) e |= 1;
  if (t > 0 && task_row[2 * t - 1] > rb) e |= 2;
  if (e) atomicOr(err, e);
}

}  // namespace gnn

using namespace gnn;

extern "C" int gnn_spmm_tasks_check(const int32_t* task_row, int64_t n_task, int64_t n_rows,
                                    int32_t* err, void* stream) {
  if (n_task < 0 || n_rows < 0 || err == nullptr || (n_task > 0 && task_row == nullptr))
    return GNN_E_ARG;
  if (n_task == 0) return GNN_OK;
  const int64_t blocks = (n_task + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffLL) return GNN_E_UNSUPPORTED;
  hipLaunchKernelGGL(spmm_tasks_check_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), task_row, n_task, n_rows, err);
  return launch_status();
}

extern "C" int gnn_spmm_csr_f32(const int64_t* rowptr, const int32_t* col, const float* val,
                                int64_t n_rows, const float* x, int64_t ldx, int64_t feat,
                                const float* bias, float* y, int64_t ldy, int64_t seg_len,
                                const int32_t* seg_row, const int64_t* seg_begin, int64_t n_seg,
                                const int32_t* long_row, const int32_t* long_seg_ptr,
                                int64_t n_long, const int32_t* small_row, const int32_t* small_col,
                                const float* small_val, int64_t n_small, const int32_t* mid_row,
                                int64_t n_mid, float* partial, uint32_t flags, void* stream) {
  return spmm_entry(rowptr, col, val, n_rows, x, ldx, feat, bias, y, ldy, seg_len, seg_row,
                    seg_begin, n_seg, long_row, long_seg_ptr, n_long, small_row, small_col,
                    small_val, n_small, mid_row, n_mid, partial, flags, stream);
}

extern "C" int gnn_spmm_csr_hub_f32(const int64_t* rowptr, const int32_t* col_hub,
                                    const float* val, int64_t n_rows, const float* x, int64_t ldx,
                                    const float* xh, int64_t ldh, int64_t feat, const float* bias,
                                    float* y, int64_t ldy, int64_t seg_len, const int32_t* seg_row,
                                    const int64_t* seg_begin, int64_t n_seg,
                                    const int32_t* long_row, const int32_t* long_seg_ptr,
                                    int64_t n_long, const int32_t* small_row,
                                    const int32_t* small_col, const float* small_val,
                                    int64_t n_small, const int32_t* mid_row, int64_t n_mid,
                                    float* partial, uint32_t flags, void* stream) {
  if (xh == nullptr) return GNN_E_ARG;
  return spmm_entry(rowptr, col_hub, val, n_rows, x, ldx, feat, bias, y, ldy, seg_len, seg_row,
                    seg_begin, n_seg, long_row, long_seg_ptr, n_long, small_row, small_col,
                    small_val, n_small, mid_row, n_mid, partial, flags, stream, xh, ldh);
}

// ---- packed row tasks (GCN/GCN.py:43-45, same aggregation): see packed_rows ----
extern "C" int gnn_spmm_csr_tasks_f32(const int64_t* rowptr, const int32_t* col, const float* val,
                                      int64_t n_rows, const float* x, int64_t ldx, const float* xh,
                                      int64_t ldh, int64_t feat, const float* bias, float* y,
                                      int64_t ldy, int64_t seg_len, const int32_t* seg_row,
                                      const int64_t* seg_begin, int64_t n_seg,
                                      const int32_t* long_row, const int32_t* long_seg_ptr,
                                      int64_t n_long, const int32_t* mid_row, int64_t n_mid,
                                      const int32_t* task_row, int64_t n_task, float* partial,
                                      uint32_t flags, void* stream) {
  if (n_task < 0 || (n_task > 0 && task_row == nullptr) || mid_row == nullptr) return GNN_E_ARG;
  if (n_task > 0x7fffffffLL) return GNN_E_UNSUPPORTED;
  if (xh == nullptr) ldh = 0;
  return spmm_entry(rowptr, col, val, n_rows, x, ldx, feat, bias, y, ldy, seg_len, seg_row,
                    seg_begin, n_seg, long_row, long_seg_ptr, n_long, nullptr, nullptr, nullptr, 0,
                    mid_row, n_mid, partial, flags, stream, xh, ldh,
                    task_row != nullptr ? task_row : mid_row, n_task);
}

// ---- pass 1 of the XCD-sliced direct form (GCN/GCN.py:43-45, same aggregation): one wave per
// item, the edge stream in scalar registers (spmm_items_kernel) ----
extern "C" int gnn_spmm_items_f32(const int64_t* rowptr, const int32_t* col, const float* val,
                                  int64_t n_pos, const float* x, int64_t ldx, int64_t feat,
                                  float* part, int64_t ldp, void* stream) {
  if (n_pos < 0 || feat < 0 || ldx < feat || ldp < feat) return GNN_E_ARG;
  if (rowptr == nullptr || x == nullptr || part == nullptr) return GNN_E_ARG;
  if (n_pos > 0 && (col == nullptr || val == nullptr)) return GNN_E_ARG;
  if (feat != 128 && feat != 256) return GNN_E_UNSUPPORTED;
  if (ldx % 4 != 0 || ldp % 4 != 0 || !aligned_to(x, 16) || !aligned_to(part, 16))
    return GNN_E_UNSUPPORTED;  // 16 B per lane
  if (ldx > 0xffffffffLL) return GNN_E_UNSUPPORTED;  // col * ldx: a 32 x 32 -> 64 bit product
  if ((n_pos + kWavesPerBlock - 1) / kWavesPerBlock > 0x7fffffffLL) return GNN_E_UNSUPPORTED;
  if (n_pos == 0) return GNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // lanes per row: at 128 columns a wave instruction gathers two rows
  return feat == 128 ? launch_spmm_items<32>(rowptr, col, val, n_pos, x, ldx, part, ldp, s)
                     : launch_spmm_items<64>(rowptr, col, val, n_pos, x, ldx, part, ldp, s);
}
