// spmm_bf16.hip -- the GCN aggregation of spmm.hip over bf16-stored feature rows:
// Y = A_hat . X (+ bias), X (and optionally the hub table xh) held as bf16, everything else
// -- val, bias, the accumulators, the partial rows of long rows, Y -- fp32.
//
// The same call site as spmm.hip, GCN/GCN.py:43-45 (torch.spmm(adj, support) + bias), with
// the support kept in the storage type torch.autocast would give it. A bf16 value is the high
// half of an fp32, so a gathered element widens exactly (a shift or a mask) and every FMA,
// shuffle reduction and epilogue after it is the fp32 kernel's (spmm_kernels.hpp): on
// bf16-rounded inputs the result is the fp32 kernel's up to the regrouping of the slot sums.
//
// Lane layout (the vector path: feat % 8 == 0, x / xh 16-B aligned, ldx / ldh % 8 == 0, the
// fp32 operands as on the fp32 vector path): one lane loads 16 B = 8 bf16 and keeps them
// packed (4 VGPRs, as an fp32x4 load) until the FMA; it owns 8 fp32 accumulators. A 256-B row
// of F = 128 is held by 16 lanes, so one wave instruction moves FOUR neighbour rows (1 KiB),
// against two 512-B rows for fp32, and the slot reduction has one xor step more. Rows wider
// than 64 lanes x 8 take 2 or 4 column chunks per lane; a launch covers 2048 columns, wider
// rows are cut into column blocks. Anything else (odd widths, views offset by one element, an
// odd row pitch) runs one element per lane with 2-B loads, 512 columns per launch.
// GNN_SPMM_BF16_VW = 4 builds the alternative layout (8-B loads, 4 bf16 per lane: the fp32
// lane count per row) for the A/B of tools/spmm_bf16_ab.py.
//
// xh has its own element type: the hub-staged form reads a bf16 table (gnn_gather_rows_bf16,
// or X itself when the hub rows are X's first rows), pass 2 of the XCD-sliced direct form
// reads pass 1's fp32 partial rows through xh. No float atomics, fixed reduction orders:
// bitwise reproducible run to run.
#include "spmm_kernels.hpp"

namespace gnn {

// out[i, :] = x[idx[i], :] for 2-byte elements (VW = 8: 16-B pieces; 1: single elements); an id
// outside [0, n_x) is not copied and raises *err
template <int VW>
__global__ __launch_bounds__(256) void gather_rows_bf16_kernel(
    const uint16_t* __restrict__ x, int64_t ldx, int64_t n_x, const int64_t* __restrict__ idx,
    int64_t n, int64_t feat, uint16_t* __restrict__ out, int64_t ldo, int32_t* __restrict__ err) {
  const int64_t nv = feat / VW;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t total = n * nv;
  for (int64_t q = t; q < total; q += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t i = q / nv, v = q % nv;
    const int64_t r = idx[i];
    if (r < 0 || r >= n_x) {
      if (v == 0) atomicOr(err, 1);
      continue;
    }
    if constexpr (VW == 8)
      *reinterpret_cast<u4*>(out + i * ldo + v * 8) =
          *reinterpret_cast<const u4*>(x + r * ldx + v * 8);
    else
      out[i * ldo + v] = x[r * ldx + v];
  }
}

static const bf16_t* as_bf16(const uint16_t* p) { return reinterpret_cast<const bf16_t*>(p); }

// xh == NULL: no hub table; xh_f32 != 0: xh holds fp32 rows, else bf16 rows
static int spmm_bf16_entry(const int64_t* rowptr, const int32_t* col, const float* val,
                           int64_t n_rows, const uint16_t* x, int64_t ldx, const void* xh,
                           int64_t ldh, int32_t xh_f32, int64_t feat, const float* bias, float* y,
                           int64_t ldy, int64_t seg_len, const int32_t* seg_row,
                           const int64_t* seg_begin, int64_t n_seg, const int32_t* long_row,
                           const int32_t* long_seg_ptr, int64_t n_long, const int32_t* small_row,
                           const int32_t* small_col, const float* small_val, int64_t n_small,
                           const int32_t* mid_row, int64_t n_mid, float* partial, uint32_t flags,
                           void* stream, const int32_t* task_row, int64_t n_task) {
  if (xh != nullptr && xh_f32)
    return spmm_entry<bf16_t, float>(rowptr, col, val, n_rows, as_bf16(x), ldx, feat, bias, y, ldy,
                                     seg_len, seg_row, seg_begin, n_seg, long_row, long_seg_ptr,
                                     n_long, small_row, small_col, small_val, n_small, mid_row,
                                     n_mid, partial, flags, stream,
                                     static_cast<const float*>(xh), ldh, task_row, n_task);
  return spmm_entry<bf16_t, bf16_t>(rowptr, col, val, n_rows, as_bf16(x), ldx, feat, bias, y, ldy,
                                    seg_len, seg_row, seg_begin, n_seg, long_row, long_seg_ptr,
                                    n_long, small_row, small_col, small_val, n_small, mid_row,
                                    n_mid, partial, flags, stream,
                                    static_cast<const bf16_t*>(xh), ldh, task_row, n_task);
}

}  // namespace gnn

using namespace gnn;

extern "C" int gnn_spmm_csr_bf16(const int64_t* rowptr, const int32_t* col, const float* val,
                                 int64_t n_rows, const uint16_t* x, int64_t ldx, int64_t feat,
                                 const float* bias, float* y, int64_t ldy, int64_t seg_len,
                                 const int32_t* seg_row, const int64_t* seg_begin, int64_t n_seg,
                                 const int32_t* long_row, const int32_t* long_seg_ptr,
                                 int64_t n_long, const int32_t* small_row,
                                 const int32_t* small_col, const float* small_val,
                                 int64_t n_small, const int32_t* mid_row, int64_t n_mid,
                                 float* partial, uint32_t flags, void* stream) {
  return spmm_bf16_entry(rowptr, col, val, n_rows, x, ldx, nullptr, 0, 0, feat, bias, y, ldy,
                         seg_len, seg_row, seg_begin, n_seg, long_row, long_seg_ptr, n_long,
                         small_row, small_col, small_val, n_small, mid_row, n_mid, partial, flags,
                         stream, nullptr, 0);
}

extern "C" int gnn_spmm_csr_hub_bf16(const int64_t* rowptr, const int32_t* col_hub,
                                     const float* val, int64_t n_rows, const uint16_t* x,
                                     int64_t ldx, const void* xh, int64_t ldh, int32_t xh_f32,
                                     int64_t feat, const float* bias, float* y, int64_t ldy,
                                     int64_t seg_len, const int32_t* seg_row,
                                     const int64_t* seg_begin, int64_t n_seg,
                                     const int32_t* long_row, const int32_t* long_seg_ptr,
                                     int64_t n_long, const int32_t* small_row,
                                     const int32_t* small_col, const float* small_val,
                                     int64_t n_small, const int32_t* mid_row, int64_t n_mid,
                                     float* partial, uint32_t flags, void* stream) {
  if (xh == nullptr || (xh_f32 != 0 && xh_f32 != 1)) return GNN_E_ARG;
  return spmm_bf16_entry(rowptr, col_hub, val, n_rows, x, ldx, xh, ldh, xh_f32, feat, bias, y, ldy,
                         seg_len, seg_row, seg_begin, n_seg, long_row, long_seg_ptr, n_long,
                         small_row, small_col, small_val, n_small, mid_row, n_mid, partial, flags,
                         stream, nullptr, 0);
}

extern "C" int gnn_spmm_csr_tasks_bf16(const int64_t* rowptr, const int32_t* col, const float* val,
                                       int64_t n_rows, const uint16_t* x, int64_t ldx,
                                       const void* xh, int64_t ldh, int32_t xh_f32, int64_t feat,
                                       const float* bias, float* y, int64_t ldy, int64_t seg_len,
                                       const int32_t* seg_row, const int64_t* seg_begin,
                                       int64_t n_seg, const int32_t* long_row,
                                       const int32_t* long_seg_ptr, int64_t n_long,
                                       const int32_t* mid_row, int64_t n_mid,
                                       const int32_t* task_row, int64_t n_task, float* partial,
                                       uint32_t flags, void* stream) {
  if (n_task < 0 || (n_task > 0 && task_row == nullptr) || mid_row == nullptr) return GNN_E_ARG;
  if (xh_f32 != 0 && xh_f32 != 1) return GNN_E_ARG;
  if (n_task > 0x7fffffffLL) return GNN_E_UNSUPPORTED;
  if (xh == nullptr) ldh = 0;
  return spmm_bf16_entry(rowptr, col, val, n_rows, x, ldx, xh, ldh, xh_f32, feat, bias, y, ldy,
                         seg_len, seg_row, seg_begin, n_seg, long_row, long_seg_ptr, n_long,
                         nullptr, nullptr, nullptr, 0, mid_row, n_mid, partial, flags, stream,
                         task_row != nullptr ? task_row : mid_row, n_task);
}

extern "C" int gnn_gather_rows_bf16(const uint16_t* x, int64_t ldx, int64_t n_x,
                                    const int64_t* idx, int64_t n, int64_t feat, uint16_t* out,
                                    int64_t ldo, int32_t* err_flag, void* stream) {
  if (n < 0 || feat < 0 || n_x < 0) return GNN_E_ARG;
  if (n == 0 || feat == 0) return GNN_OK;
  if (!x || !idx || !out || !err_flag || ldx < feat || ldo < feat) return GNN_E_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec8 = feat % 8 == 0 && ldx % 8 == 0 && ldo % 8 == 0 && aligned_to(x, 16) &&
                    aligned_to(out, 16);
  const int64_t total = n * (vec8 ? feat / 8 : feat);
  const int64_t blocks = total / 256 + 1 < 65536 ? total / 256 + 1 : 65536;
  if (vec8)
    hipLaunchKernelGGL(gather_rows_bf16_kernel<8>, dim3(static_cast<unsigned>(blocks)), dim3(256),
                       0, s, x, ldx, n_x, idx, n, feat, out, ldo, err_flag);
  else
    hipLaunchKernelGGL(gather_rows_bf16_kernel<1>, dim3(static_cast<unsigned>(blocks)), dim3(256),
                       0, s, x, ldx, n_x, idx, n, feat, out, ldo, err_flag);
  return launch_status();
}
