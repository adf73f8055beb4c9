// sage_bf16.hip -- the GraphSAGE aggregation of sage.hip over a bf16-stored feature table (or
// pre-gathered neighbour tensor): fp32 sums, fp32 / int64 outputs.
//
// The same call sites as sage.hip -- Aggregator (GraphSAGE/graph_utils.py:4-11), the
// torch.embedding gathers of GraphSAGE/GraphSAGE.py:47-49 and the cat[self, agg] of :17 --
// with the node feature table kept in 2 bytes per element: the largest object a GraphSAGE user
// holds, and the bytes the layer-0 gather moves. A bf16 value is the high half of an fp32, so a
// loaded element widens exactly and in order: MEAN / SUM accumulate in fp32 as the fp32 kernel
// does, MAXPOOL and ARGMAX are exact functions of the stored values (first maximum, a NaN
// counts as the maximum), and the centre rows of the concat form are written widened into the
// fp32 [self | agg] buffer the GEMM reads. Every instruction after the load is the fp32
// kernel's (sage_kernels.hpp).
//
// Lane layout (the vector path: feat % 8 == 0, every table / neighbour pitch % 8 == 0, the
// base 16-B aligned; outputs as on the fp32 vector path: pitch % 4 == 0, 16-B aligned fp32,
// 32-B aligned int64): one lane loads 16 B = 8 bf16 and keeps them packed (4 VGPRs) for the U
// slots in flight, widening at the use; it owns 8 fp32 accumulators (and 8 argmax indices,
// stored as four 16-B pairs of int64). A 256-B row of F = 128 is held by 16 lanes, so one wave
// instruction moves FOUR neighbour rows, against two 512-B rows for fp32, and the slot combine
// has one xor step more. Rows wider than 64 lanes x 8 take 2, 4 or 8 column chunks per lane; a
// launch covers 512 vectors = 4096 columns, wider rows are cut into column blocks. Anything
// else (odd widths, views offset by one element, an odd pitch) runs one element per lane with
// 2-B loads, 512 columns per launch.
#include "sage_kernels.hpp"

namespace gnn {

// out_f32[i, :] = widen(x_bf16[idx[i], :])  (VW = 8: one 16-B load, two 16-B stores per lane;
// 1: single elements); an id outside [0, n_x) is not copied and raises *err
template <int VW>
__global__ __launch_bounds__(256) void gather_rows_widen_kernel(
    const bf16_t* __restrict__ x, int64_t ldx, int64_t n_x, const int64_t* __restrict__ idx,
    int64_t n, int64_t feat, float* __restrict__ out, int64_t ldo, int32_t* __restrict__ err) {
  typedef Row<bf16_t, VW> RX;
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
    vstore<VW>(out + i * ldo + v * VW, RX::f32(RX::load(x + r * ldx + v * VW)));
  }
}

static const bf16_t* as_bf16(const uint16_t* p) { return reinterpret_cast<const bf16_t*>(p); }

}  // namespace gnn

using namespace gnn;

extern "C" int gnn_sage_aggregate_bf16(const uint16_t* neigh, int64_t ld_k, int64_t ld_m,
                                       int64_t M, int64_t k, int64_t feat, int32_t mode,
                                       void* out, int64_t ldo, void* stream) {
  return sage_aggregate_entry<bf16_t>(as_bf16(neigh), ld_k, ld_m, M, k, feat, mode, out, ldo,
                                      stream);
}

extern "C" int gnn_sage_gather_aggregate_bf16(const uint16_t* table, int64_t ldt, int64_t n_table,
                                              const int64_t* idx, int64_t ldi, int64_t M,
                                              int64_t k, int64_t feat, int32_t mode, void* out,
                                              int64_t ldo, int32_t* err_flag, void* stream) {
  return sage_gather_aggregate_entry<bf16_t>(as_bf16(table), ldt, n_table, idx, ldi, M, k, feat,
                                             mode, out, ldo, err_flag, stream);
}

extern "C" int gnn_sage_gather_concat_live_bf16(const uint16_t* table, int64_t ldt,
                                                int64_t n_table, const int64_t* self_idx,
                                                const int64_t* idx, int64_t ldi, int64_t M,
                                                const int64_t* live, int64_t k, int64_t feat,
                                                int32_t mode, float* self_out, int64_t ld_self,
                                                float* out, int64_t ldo, int32_t* err_flag,
                                                void* stream) {
  return sage_gather_concat_entry<bf16_t>(as_bf16(table), ldt, n_table, self_idx, idx, ldi, M,
                                          live, k, feat, mode, self_out, ld_self, out, ldo,
                                          err_flag, stream);
}

extern "C" int gnn_sage_gather_concat_bf16(const uint16_t* table, int64_t ldt, int64_t n_table,
                                           const int64_t* self_idx, const int64_t* idx,
                                           int64_t ldi, int64_t M, int64_t k, int64_t feat,
                                           int32_t mode, float* self_out, int64_t ld_self,
                                           float* out, int64_t ldo, int32_t* err_flag,
                                           void* stream) {
  return gnn_sage_gather_concat_live_bf16(table, ldt, n_table, self_idx, idx, ldi, M, nullptr, k,
                                          feat, mode, self_out, ld_self, out, ldo, err_flag,
                                          stream);
}

extern "C" int gnn_gather_rows_bf16_f32(const uint16_t* x, int64_t ldx, int64_t n_x,
                                        const int64_t* idx, int64_t n, int64_t feat, float* out,
                                        int64_t ldo, int32_t* err_flag, void* stream) {
  if (n < 0 || feat < 0 || n_x < 0) return GNN_E_ARG;
  if (n == 0 || feat == 0) return GNN_OK;
  if (!x || !idx || !out || !err_flag || ldx < feat || ldo < feat) return GNN_E_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec8 = feat % 8 == 0 && ldx % 8 == 0 && ldo % 4 == 0 && aligned_to(x, 16) &&
                    aligned_to(out, 16);
  const int64_t total = n * (vec8 ? feat / 8 : feat);
  const int64_t blocks = total / 256 + 1 < 65536 ? total / 256 + 1 : 65536;
  if (vec8)
    hipLaunchKernelGGL(gather_rows_widen_kernel<8>, dim3(static_cast<unsigned>(blocks)), dim3(256),
                       0, s, as_bf16(x), ldx, n_x, idx, n, feat, out, ldo, err_flag);
  else
    hipLaunchKernelGGL(gather_rows_widen_kernel<1>, dim3(static_cast<unsigned>(blocks)), dim3(256),
                       0, s, as_bf16(x), ldx, n_x, idx, n, feat, out, ldo, err_flag);
  return launch_status();
}

extern "C" int gnn_sage_gather_concat_arg_bf16(const uint16_t* table, int64_t ldt, int64_t n_table,
                                               const int64_t* self_idx, const int64_t* idx,
                                               int64_t ldi, int64_t M, int64_t k, int64_t feat,
                                               float* self_out, int64_t ld_self, float* out,
                                               int64_t ldo, uint8_t* arg, int64_t lda,
                                               int32_t* err_flag, void* stream) {
  return sage_gather_concat_arg_entry<bf16_t>(as_bf16(table), ldt, n_table, self_idx, idx, ldi, M,
                                              k, feat, self_out, ld_self, out, ldo, arg, lda,
                                              err_flag, stream);
}

extern "C" int gnn_sage_gather_aggregate_live_bf16(const uint16_t* table, int64_t ldt,
                                                   int64_t n_table, const int64_t* idx,
                                                   int64_t ldi, int64_t M, const int64_t* live,
                                                   int64_t k, int64_t feat, int32_t mode,
                                                   float* out, int64_t ldo, int32_t* err_flag,
                                                   void* stream) {
  return sage_gather_aggregate_live_entry<bf16_t>(as_bf16(table), ldt, n_table, idx, ldi, M, live,
                                                  k, feat, mode, out, ldo, err_flag, stream);
}

extern "C" int gnn_sage_gather_aggregate_arg_bf16(const uint16_t* table, int64_t ldt,
                                                  int64_t n_table, const int64_t* idx, int64_t ldi,
                                                  int64_t M, int64_t k, int64_t feat, float* out,
                                                  int64_t ldo, uint8_t* arg, int64_t lda,
                                                  int32_t* err_flag, void* stream) {
  return sage_gather_aggregate_arg_entry<bf16_t>(as_bf16(table), ldt, n_table, idx, ldi, M, k, feat,
                                                 out, ldo, arg, lda, err_flag, stream);
}
