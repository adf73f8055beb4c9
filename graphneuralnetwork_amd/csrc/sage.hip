// sage.hip -- GraphSAGE neighbour aggregation + row gathers on gfx950.
//
// Replaces
//   Aggregator(neigh_feat, 'MEAN' | 'MAX')         GraphSAGE/graph_utils.py:4-11
//     MEAN -> torch.mean(neigh_feat, dim=1)         (fp32 [M, F])
//     MAX  -> torch.argmax(neigh_feat, dim=1)       (int64 [M, F]: FIRST maximal position,
//                                                    a NaN counts as the maximum)
//   value max-pool (north_star "mean/max-pool")     torch.max(neigh, dim=1).values, the
//     value NeighborAggregator 'max' reaches for      (GraphSAGE_Pytorch/models/Aggregator.py:23-24):
//                                                    fp32 [M, F], a NaN in the slice propagates
//   torch.embedding(feats_data, index_map)          GraphSAGE/GraphSAGE.py:47-49,
//                                                    GraphSAGE/data_utils.py:161-162
// Two input forms:
//   pre-gathered  neigh_feat [M, k, F] (the layer-0 tensor collate_fn builds);
//   fused gather  table [n, F] + index map [M, k] int64: the (M, k, F) tensor the
//                 reference materialises with torch.embedding is never written --
//                 every neighbour row is read once from the table and reduced in
//                 registers (K7/K8 + K9 of SURVEY 2.3).
// The aggregation kernel and its dispatch are generic over the table's element type
// (sage_kernels.hpp); this file holds the fp32 instances and C entries, sage_bf16.hip those
// over a bf16-stored table.
#include "sage_kernels.hpp"

namespace gnn {

// out[i, :] = x[idx[i], :]  (torch.embedding / halo send-buffer packing)
template <int VW>
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ x, int64_t ldx,
                                                         int64_t n_x, const int64_t* __restrict__ idx,
                                                         int64_t n, int64_t feat,
                                                         float* __restrict__ out, int64_t ldo,
                                                         int32_t* __restrict__ err) {
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
    vstore<VW>(out + i * ldo + v * VW, vload<VW>(x + r * ldx + v * VW));
  }
}

// out[i, c] = keep(seed, key, c) ? x[r, c] / (1 - p) : x[r, c] * 0 (torch's x * mask * scale:
// NaN stays NaN) with r = idx ? idx[i] : i and key = r
// (KEY_SRC) or i: F.dropout (GAT/models/GAT.py:15,17) as a hashed element mask, fused with the
// models' relabelling gather. The mask is never stored: the backward re-derives it from the
// seed (the same launch with key = the source row through the inverse permutation).
template <int VW, bool KEY_SRC>
__global__ __launch_bounds__(256) void dropout_rows_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t n_x, const int64_t* __restrict__ idx,
    int64_t n, int64_t feat, float p, float scale, uint64_t seed, float* __restrict__ out,
    int64_t ldo, int32_t* __restrict__ err) {
  const int64_t nv = feat / VW;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t total = n * nv;
  for (int64_t q = t; q < total; q += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const int64_t i = q / nv, v = q % nv;
    const int64_t r = idx ? idx[i] : i;
    if (r < 0 || r >= n_x) {
      if (v == 0) atomicOr(err, 1);
      continue;
    }
    const int64_t key = KEY_SRC ? r : i;
    typename Vec<VW>::T a = vload<VW>(x + r * ldx + v * VW);
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const int c = static_cast<int>(v * VW + j);
      vset(a, j, dropout_keep(seed, key, c, p) ? vget(a, j) * scale : vget(a, j) * 0.f);
    }
    vstore<VW>(out + i * ldo + v * VW, a);
  }
}

}  // namespace gnn

using namespace gnn;

extern "C" int gnn_sage_aggregate_f32(const float* neigh, int64_t ld_k, int64_t ld_m, int64_t M,
                                      int64_t k, int64_t feat, int32_t mode, void* out,
                                      int64_t ldo, void* stream) {
  return sage_aggregate_entry<float>(neigh, ld_k, ld_m, M, k, feat, mode, out, ldo, stream);
}

extern "C" int gnn_sage_gather_aggregate_f32(const float* table, int64_t ldt, int64_t n_table,
                                             const int64_t* idx, int64_t ldi, int64_t M, int64_t k,
                                             int64_t feat, int32_t mode, void* out, int64_t ldo,
                                             int32_t* err_flag, void* stream) {
  return sage_gather_aggregate_entry<float>(table, ldt, n_table, idx, ldi, M, k, feat, mode, out,
                                            ldo, err_flag, stream);
}

extern "C" int gnn_gather_rows_f32(const float* x, int64_t ldx, int64_t n_x, const int64_t* idx,
                                   int64_t n, int64_t feat, float* out, int64_t ldo,
                                   int32_t* err_flag, void* stream) {
  if (n < 0 || feat < 0 || n_x < 0) return GNN_E_ARG;
  if (n == 0 || feat == 0) return GNN_OK;
  if (!x || !idx || !out || !err_flag || ldx < feat || ldo < feat) return GNN_E_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec4 = feat % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && aligned_to(x, 16) &&
                    aligned_to(out, 16);
  const int64_t total = n * (vec4 ? feat / 4 : feat);
  const int64_t blocks = total / 256 + 1 < 65536 ? total / 256 + 1 : 65536;
  if (vec4)
    hipLaunchKernelGGL(gather_rows_kernel<4>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s,
                       x, ldx, n_x, idx, n, feat, out, ldo, err_flag);
  else
    hipLaunchKernelGGL(gather_rows_kernel<1>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s,
                       x, ldx, n_x, idx, n, feat, out, ldo, err_flag);
  return launch_status();
}

extern "C" int gnn_dropout_rows_f32(const float* x, int64_t ldx, int64_t n_x, const int64_t* idx,
                                    int32_t key_by_source, int64_t n, int64_t feat, float p,
                                    uint64_t seed, float* out, int64_t ldo, int32_t* err_flag,
                                    void* stream) {
  if (n < 0 || feat < 0 || n_x < 0 || !(p >= 0.f && p < 1.f)) return GNN_E_ARG;
  if (feat > 0x7fffffff) return GNN_E_ARG;  // the hash takes the column as an int
  if (n == 0 || feat == 0) return GNN_OK;
  if (!x || !out || !err_flag || ldx < feat || ldo < feat) return GNN_E_ARG;
  if (!idx && n > n_x) return GNN_E_ARG;
  if (x == out && idx) return GNN_E_ARG;  // in place only without a gather
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec4 = feat % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && aligned_to(x, 16) &&
                    aligned_to(out, 16);
  const float scale = 1.0f / (1.0f - p);
  const int64_t total = n * (vec4 ? feat / 4 : feat);
  const int64_t blocks = total / 256 + 1 < 65536 ? total / 256 + 1 : 65536;
  const dim3 grid(static_cast<unsigned>(blocks));
  const bool ks = key_by_source != 0;
  if (vec4 && ks)
    hipLaunchKernelGGL((dropout_rows_kernel<4, true>), grid, dim3(256), 0, s, x, ldx, n_x, idx, n,
                       feat, p, scale, seed, out, ldo, err_flag);
  else if (vec4)
    hipLaunchKernelGGL((dropout_rows_kernel<4, false>), grid, dim3(256), 0, s, x, ldx, n_x, idx, n,
                       feat, p, scale, seed, out, ldo, err_flag);
  else if (ks)
    hipLaunchKernelGGL((dropout_rows_kernel<1, true>), grid, dim3(256), 0, s, x, ldx, n_x, idx, n,
                       feat, p, scale, seed, out, ldo, err_flag);
  else
    hipLaunchKernelGGL((dropout_rows_kernel<1, false>), grid, dim3(256), 0, s, x, ldx, n_x, idx, n,
                       feat, p, scale, seed, out, ldo, err_flag);
  return launch_status();
}

extern "C" int gnn_sage_gather_concat_live_f32(const float* table, int64_t ldt, int64_t n_table,
                                               const int64_t* self_idx, const int64_t* idx,
                                               int64_t ldi, int64_t M, const int64_t* live,
                                               int64_t k, int64_t feat, int32_t mode,
                                               float* self_out, int64_t ld_self, float* out,
                                               int64_t ldo, int32_t* err_flag, void* stream);

extern "C" int gnn_sage_gather_concat_f32(const float* table, int64_t ldt, int64_t n_table,
                                          const int64_t* self_idx, const int64_t* idx, int64_t ldi,
                                          int64_t M, int64_t k, int64_t feat, int32_t mode,
                                          float* self_out, int64_t ld_self, float* out, int64_t ldo,
                                          int32_t* err_flag, void* stream) {
  return gnn_sage_gather_concat_live_f32(table, ldt, n_table, self_idx, idx, ldi, M, nullptr, k,
                                         feat, mode, self_out, ld_self, out, ldo, err_flag, stream);
}

extern "C" int gnn_sage_gather_concat_live_f32(const float* table, int64_t ldt, int64_t n_table,
                                               const int64_t* self_idx, const int64_t* idx,
                                               int64_t ldi, int64_t M, const int64_t* live,
                                               int64_t k, int64_t feat, int32_t mode,
                                               float* self_out, int64_t ld_self, float* out,
                                               int64_t ldo, int32_t* err_flag, void* stream) {
  return sage_gather_concat_entry<float>(table, ldt, n_table, self_idx, idx, ldi, M, live, k, feat,
                                         mode, self_out, ld_self, out, ldo, err_flag, stream);
}

extern "C" int gnn_sage_gather_concat_arg_supported(int64_t feat, int64_t k) {
  return sage_concat_arg_shape(feat, k);
}

extern "C" int gnn_sage_gather_concat_arg_f32(const float* table, int64_t ldt, int64_t n_table,
                                              const int64_t* self_idx, const int64_t* idx,
                                              int64_t ldi, int64_t M, int64_t k, int64_t feat,
                                              float* self_out, int64_t ld_self, float* out,
                                              int64_t ldo, uint8_t* arg, int64_t lda,
                                              int32_t* err_flag, void* stream) {
  return sage_gather_concat_arg_entry<float>(table, ldt, n_table, self_idx, idx, ldi, M, k, feat,
                                             self_out, ld_self, out, ldo, arg, lda, err_flag,
                                             stream);
}

// ---- the gcn-mode SageLayer (GraphSAGE/GraphSAGE.py:13-14: Linear over the aggregate alone) ----
extern "C" int gnn_sage_gather_aggregate_live_f32(const float* table, int64_t ldt, int64_t n_table,
                                                  const int64_t* idx, int64_t ldi, int64_t M,
                                                  const int64_t* live, int64_t k, int64_t feat,
                                                  int32_t mode, float* out, int64_t ldo,
                                                  int32_t* err_flag, void* stream) {
  return sage_gather_aggregate_live_entry<float>(table, ldt, n_table, idx, ldi, M, live, k, feat,
                                                 mode, out, ldo, err_flag, stream);
}

extern "C" int gnn_sage_gather_aggregate_arg_supported(int64_t feat, int64_t k) {
  return sage_concat_arg_shape(feat, k);
}

extern "C" int gnn_sage_gather_aggregate_arg_f32(const float* table, int64_t ldt, int64_t n_table,
                                                 const int64_t* idx, int64_t ldi, int64_t M,
                                                 int64_t k, int64_t feat, float* out, int64_t ldo,
                                                 uint8_t* arg, int64_t lda, int32_t* err_flag,
                                                 void* stream) {
  return sage_gather_aggregate_arg_entry<float>(table, ldt, n_table, idx, ldi, M, k, feat, out, ldo,
                                                arg, lda, err_flag, stream);
}
