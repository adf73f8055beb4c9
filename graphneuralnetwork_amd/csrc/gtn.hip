// gtn.hip -- the numeric side of a Graph Transformer Network on CSR patterns.
//
// The reference's GTN (GTN/models/GTLayer.py:25,30 torch.bmm of dense [C, N, N] stacks;
// GTN/models/GTN.py:49-52 a dense mm per channel) restated as VALUES over FIXED patterns:
// the structure of every product is known beforehand (hetero.relation_product), so what is
// left is
//   gnn_masked_product_f32   the values of a sparse product on a given pattern P, C value
//                            sets (channels) in one walk of the structure, two modes;
//   gnn_edge_aggregate_f32   Y[c, r, :] = sum_e v[c, e] X[c * x_stride + col_e, :];
//   gnn_edge_dot_f32         dv[c, e] = <G[c, row_e, :], X[col_e, :]>;
//   gnn_edge_rowsum_f32      d[c, r] = sum_e v[c, e]  (the column sums of norm / gcn_conv,
//                            run over the column view).
// Everything is fp32 with 64-bit offsets and NO float atomics: every output element is
// written once, by one lane, after a sum in the operand's stored order, so results are
// bit-identical from run to run.
//
// The masked product is output-stationary. A wavefront takes 64 consecutive entries of P:
//   lane class  (walked row <= kMpLaneMax entries) the entry's own lane walks the row;
//   wave class  (longer) the wavefront takes such entries one after another, its lanes
//               across 64 walked entries at a time: every lane searches for its entry, and
//               the hits are then added in ascending lane order (a ballot, lowest bit first)
//               -- the walked row's stored order again, so both classes give the same bits.
// The position found by the binary search is used for all C channels.
#include "common.hpp"
#include "host.hpp"

namespace gnn {

constexpr int kMpLaneMax = 32;  // walked rows up to this length are summed by one lane
constexpr int kMpBlock = 256;
constexpr int kMpMaxC = 8;
constexpr int kMpGrid = 1 << 16;  // workgroups at most; a wavefront strides over P
constexpr int64_t kMpDimLimit = 0x7fffffffLL;
constexpr int kEaBlock = 256;

struct MpWs {
  int32_t* err;
  int64_t bytes;
};

static MpWs mp_carve(void* ws) {
  Carve c{static_cast<char*>(ws)};
  MpWs w{};
  w.err = c.take<int32_t>(1);
  w.bytes = c.used;
  return w;
}

// One thread per row: the rowptr span inside [0, nnz] and ordered, every id inside [0, cols)
// and, for an operand that is searched, strictly ascending within the row.
__global__ void mp_validate_kernel(const int64_t* __restrict__ rowptr,
                                   const int32_t* __restrict__ col, int64_t rows, int64_t cols,
                                   int64_t nnz, int ascending, int32_t* __restrict__ err) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  bool bad = false;
  if (i == 0) bad = rowptr[0] != 0 || rowptr[rows] != nnz;
  if (i < rows) {
    const int64_t a = rowptr[i], b = rowptr[i + 1];
    if (a > b || a < 0 || b > nnz) {
      bad = true;
    } else {
      int32_t prev = -1;
      for (int64_t e = a; e < b; ++e) {
        const int32_t c = col[e];
        bad = bad || c < 0 || c >= cols || (ascending && c <= prev);
        prev = c;
      }
    }
  }
  if (bad) atomicOr(err, 1);
}

// first position in [lo, hi) whose id is >= key (ids strictly ascending)
__device__ __forceinline__ int64_t mp_lower_bound(const int32_t* __restrict__ col, int64_t lo,
                                                  int64_t hi, int32_t key) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (col[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the row of entry e: the largest r in [0, rows) with rowptr[r] <= e (rows >= 1, e < nnz)
__device__ __forceinline__ int64_t row_of_entry(const int64_t* __restrict__ rowptr, int64_t rows,
                                                int64_t e) {
  int64_t lo = 0, hi = rows;  // the answer is in [lo, hi)
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (rowptr[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The walked entry q of P entry (r, s): the position of its partner in the searched operand, or
// -1. MODE 0 walks A's row r and searches B's row col_A[q] for s; MODE 1 walks B's row s and
// searches A's row r ([l_lo, l_hi)) for col_B[q].
template <int MODE>
__device__ __forceinline__ int64_t mp_partner(const int32_t* __restrict__ acol,
                                              const int64_t* __restrict__ brp,
                                              const int32_t* __restrict__ bcol, int64_t q,
                                              int32_t s, int64_t l_lo, int64_t l_hi) {
  if (MODE == 0) {
    const int32_t kk = acol[q];
    const int64_t hi = brp[kk + 1];
    const int64_t pos = mp_lower_bound(bcol, brp[kk], hi, s);
    return (pos < hi && bcol[pos] == s) ? pos : -1;
  } else {
    const int32_t key = bcol[q];
    const int64_t pos = mp_lower_bound(acol, l_lo, l_hi, key);
    return (pos < l_hi && acol[pos] == key) ? pos : -1;
  }
}

template <int MODE, int C>
__global__ __launch_bounds__(kMpBlock) void mp_kernel(
    const int64_t* __restrict__ arp, const int32_t* __restrict__ acol,
    const float* __restrict__ aval, int64_t nnz_a, const int64_t* __restrict__ brp,
    const int32_t* __restrict__ bcol, const float* __restrict__ bval, int64_t nnz_b,
    const int64_t* __restrict__ prp, const int32_t* __restrict__ pcol, int64_t nnz_p, int64_t n,
    float* __restrict__ out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * (kMpBlock / kWave) + (threadIdx.x >> 6);
  const int64_t n_waves = static_cast<int64_t>(gridDim.x) * (kMpBlock / kWave);
  // the walked operand's values w, the searched operand's values l
  const float* __restrict__ wv = MODE == 0 ? aval : bval;
  const float* __restrict__ lv = MODE == 0 ? bval : aval;
  const int64_t w_nnz = MODE == 0 ? nnz_a : nnz_b, l_nnz = MODE == 0 ? nnz_b : nnz_a;
  for (int64_t base = wave * kWave; base < nnz_p; base += n_waves * kWave) {
    const int64_t e = base + lane;
    const bool valid = e < nnz_p;
    int64_t w_lo = 0, w_hi = 0, l_lo = 0, l_hi = 0;
    int32_t s = 0;
    if (valid) {
      const int64_t r = row_of_entry(prp, n, e);
      s = pcol[e];
      if (MODE == 0) {
        w_lo = arp[r];
        w_hi = arp[r + 1];
      } else {
        w_lo = brp[s];
        w_hi = brp[s + 1];
        l_lo = arp[r];
        l_hi = arp[r + 1];
      }
    }
    const int64_t len = w_hi - w_lo;
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    if (len <= kMpLaneMax) {
      for (int64_t q = w_lo; q < w_hi; ++q) {
        const int64_t pos = mp_partner<MODE>(acol, brp, bcol, q, s, l_lo, l_hi);
        if (pos >= 0) {
#pragma unroll
          for (int c = 0; c < C; ++c)
            acc[c] = __fmaf_rn(wv[c * w_nnz + q], lv[c * l_nnz + pos], acc[c]);
        }
      }
    }
    uint64_t heavy = __ballot(len > kMpLaneMax);
    while (heavy) {
      const int j = __ffsll(static_cast<unsigned long long>(heavy)) - 1;
      heavy &= heavy - 1;
      const int64_t jw_lo = __shfl(w_lo, j, kWave), jw_hi = __shfl(w_hi, j, kWave);
      const int64_t jl_lo = __shfl(l_lo, j, kWave), jl_hi = __shfl(l_hi, j, kWave);
      const int32_t js = __shfl(s, j, kWave);
      float sum[C];  // the same on every lane
#pragma unroll
      for (int c = 0; c < C; ++c) sum[c] = 0.f;
      for (int64_t c0 = jw_lo; c0 < jw_hi; c0 += kWave) {
        const int64_t q = c0 + lane;
        float tw[C], tl[C];
        bool hit = false;
        if (q < jw_hi) {
          const int64_t pos = mp_partner<MODE>(acol, brp, bcol, q, js, jl_lo, jl_hi);
          if (pos >= 0) {
            hit = true;
#pragma unroll
            for (int c = 0; c < C; ++c) {
              tw[c] = wv[c * w_nnz + q];
              tl[c] = lv[c * l_nnz + pos];
            }
          }
        }
        if (!hit) {
#pragma unroll
          for (int c = 0; c < C; ++c) tw[c] = tl[c] = 0.f;
        }
        uint64_t hits = __ballot(hit);
        while (hits) {  // ascending lanes: the walked row's stored order
          const int t = __ffsll(static_cast<unsigned long long>(hits)) - 1;
          hits &= hits - 1;
#pragma unroll
          for (int c = 0; c < C; ++c)
            sum[c] = __fmaf_rn(__shfl(tw[c], t, kWave), __shfl(tl[c], t, kWave), sum[c]);
        }
      }
      if (lane == j) {
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = sum[c];
      }
    }
    if (valid) {
#pragma unroll
      for (int c = 0; c < C; ++c) out[c * nnz_p + e] = acc[c];
    }
  }
}

// ------------------------------------------------------------------------ edge aggregate
// G = 2^lg lanes per row, a float4 of the feature row each, all C channels; the row's edges one
// after another in CSR order.
template <int C>
__global__ __launch_bounds__(kEaBlock) void ea_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, int64_t nnz, int64_t n_rows, const float* __restrict__ X,
    int64_t ldx, int64_t x_stride, float* __restrict__ Y, int64_t ldy, int F, int lg,
    int skip_diag) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kEaBlock + threadIdx.x;
  const int64_t r = t >> lg;
  const int f = static_cast<int>(t & ((1 << lg) - 1)) * 4;
  if (r >= n_rows || f >= F) return;
  f4 acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = vzero<4>();
  const int64_t e_end = rowptr[r + 1];
  for (int64_t e = rowptr[r]; e < e_end; ++e) {
    const int64_t j = col[e];
    if (skip_diag && j == r) continue;
    if (x_stride == 0) {
      const f4 x = vload<4>(X + j * ldx + f);
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += val[c * nnz + e] * x;
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c)
        acc[c] += val[c * nnz + e] * vload<4>(X + (c * x_stride + j) * ldx + f);
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) vstore<4>(Y + (c * n_rows + r) * ldy + f, acc[c]);
}

// ----------------------------------------------------------------------------- edge dot
// G = 2^lg lanes per edge: a float4 of X's row (read once for all channels) against the same
// float4 of each channel's G row, then a fixed xor-shuffle sum over the group.
template <int C>
__global__ __launch_bounds__(kEaBlock) void ed_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t nnz,
    int64_t n_rows, const float* __restrict__ Gd, int64_t ldg, const float* __restrict__ X,
    int64_t ldx, float* __restrict__ dv, int F, int lg, int skip_diag) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kEaBlock + threadIdx.x;
  const int64_t e = t >> lg;
  const int lig = static_cast<int>(t & ((1 << lg) - 1));
  const bool valid = e < nnz;  // the same for a whole group; every lane stays for the shuffles
  int64_t r = 0, j = 0;
  if (valid) {
    r = row_of_entry(rowptr, n_rows, e);
    j = col[e];
  }
  const bool live = valid && lig * 4 < F && !(skip_diag && j == r);
  const f4 x = live ? vload<4>(X + j * ldx + lig * 4) : vzero<4>();
  float p[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const f4 g = live ? vload<4>(Gd + (c * n_rows + r) * ldg + lig * 4) : vzero<4>();
    p[c] = __fmaf_rn(g.w, x.w, __fmaf_rn(g.z, x.z, __fmaf_rn(g.y, x.y, g.x * x.x)));
  }
  for (int o = (1 << lg) >> 1; o > 0; o >>= 1) {
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] += __shfl_xor(p[c], o, kWave);
  }
  if (valid && lig == 0) {
#pragma unroll
    for (int c = 0; c < C; ++c) dv[c * nnz + e] = p[c];
  }
}

// one thread per (channel, row): the row's values added in CSR order
__global__ void ers_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                           const float* __restrict__ val, int64_t nnz, int64_t n_rows, int C,
                           int skip_diag, float* __restrict__ y) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= n_rows * C) return;
  const int64_t c = t / n_rows, r = t - c * n_rows;
  float acc = 0.f;
  const int64_t e_end = rowptr[r + 1];
  for (int64_t e = rowptr[r]; e < e_end; ++e)
    if (!(skip_diag && col[e] == r)) acc += val[c * nnz + e];
  y[t] = acc;
}

static int mp_check_dims(int mode, int64_t n, int64_t k, int64_t m, int64_t nnz_a, int64_t nnz_b,
                         int64_t nnz_p, int C) {
  if (n < 0 || k < 0 || m < 0 || nnz_a < 0 || nnz_b < 0 || nnz_p < 0 || (mode != 0 && mode != 1))
    return GNN_E_ARG;
  if (C < 1 || C > kMpMaxC || n >= kMpDimLimit || k >= kMpDimLimit || m >= kMpDimLimit)
    return GNN_E_UNSUPPORTED;
  return GNN_OK;
}

// feature rows of the edge kernels: F % 4 == 0, 4 <= F <= 256, 16-byte aligned rows
static int edge_check_rows(int64_t F, int C) {
  if (C < 1 || C > kMpMaxC || F < 4 || F > 256 || F % 4 != 0) return GNN_E_UNSUPPORTED;
  return GNN_OK;
}
static int edge_lanes_log2(int64_t F) {
  int lg = 0;
  while ((4 << lg) < F) ++lg;
  return lg;  // 2^lg float4 lanes cover F, <= 64
}

#define GNN_PER_CHANNELS(C, CALL) \
  switch (C) {                    \
    case 1: CALL(1); break;       \
    case 2: CALL(2); break;       \
    case 3: CALL(3); break;       \
    case 4: CALL(4); break;       \
    case 5: CALL(5); break;       \
    case 6: CALL(6); break;       \
    case 7: CALL(7); break;       \
    default: CALL(8); break;      \
  }

}  // namespace gnn

using namespace gnn;

extern "C" int64_t gnn_masked_product_workspace_bytes(int64_t n, int64_t k, int64_t m,
                                                      int64_t nnz_a, int64_t nnz_b,
                                                      int64_t nnz_p, int C) {
  const int rc = mp_check_dims(0, n, k, m, nnz_a, nnz_b, nnz_p, C);
  if (rc != GNN_OK) return rc;
  return mp_carve(nullptr).bytes;
}

extern "C" int gnn_masked_product_class_limits(int64_t* lane_max, int64_t* wave_chunk) {
  if (!lane_max || !wave_chunk) return GNN_E_ARG;
  *lane_max = kMpLaneMax;
  *wave_chunk = kWave;
  return GNN_OK;
}

extern "C" int gnn_masked_product_f32(int mode, const int64_t* a_rowptr, const int32_t* a_col,
                                      const float* a_val, int64_t nnz_a,
                                      const int64_t* b_rowptr, const int32_t* b_col,
                                      const float* b_val, int64_t nnz_b,
                                      const int64_t* p_rowptr, const int32_t* p_col,
                                      int64_t nnz_p, int64_t n, int64_t k, int64_t m, int C,
                                      float* out, int validate, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  const int rc = mp_check_dims(mode, n, k, m, nnz_a, nnz_b, nnz_p, C);
  if (rc != GNN_OK) return rc;
  if (!a_rowptr || !b_rowptr || !p_rowptr || !workspace || (nnz_a > 0 && (!a_col || !a_val)) ||
      (nnz_b > 0 && (!b_col || !b_val)) || (nnz_p > 0 && (!p_col || !out || n == 0)))
    return GNN_E_ARG;
  MpWs w = mp_carve(workspace);
  if (workspace_bytes < w.bytes) return GNN_E_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t b_rows = mode == 0 ? k : m, b_cols = mode == 0 ? m : k;
  if (validate) {
    GNN_TRY(hipMemsetAsync(w.err, 0, sizeof(int32_t), s));
    hipLaunchKernelGGL(mp_validate_kernel, dim3(blocks(n + 1, 256)), dim3(256), 0, s, a_rowptr,
                       a_col, n, k, nnz_a, mode == 1, w.err);
    hipLaunchKernelGGL(mp_validate_kernel, dim3(blocks(b_rows + 1, 256)), dim3(256), 0, s,
                       b_rowptr, b_col, b_rows, b_cols, nnz_b, mode == 0, w.err);
    hipLaunchKernelGGL(mp_validate_kernel, dim3(blocks(n + 1, 256)), dim3(256), 0, s, p_rowptr,
                       p_col, n, m, nnz_p, 0, w.err);
    int32_t herr = 0;
    GNN_TRY(sync_read(w.err, &herr, 1, s));
    if (herr) return GNN_E_ARG;  // nothing is read through a malformed operand
  }
  if (nnz_p == 0) return launch_status();
  const int64_t want = (nnz_p + kMpBlock - 1) / kMpBlock;
  const unsigned grid = static_cast<unsigned>(want < kMpGrid ? want : kMpGrid);
#define MP_LAUNCH(CC)                                                                          \
  do {                                                                                         \
    if (mode == 0)                                                                             \
      hipLaunchKernelGGL((mp_kernel<0, CC>), dim3(grid), dim3(kMpBlock), 0, s, a_rowptr, a_col, \
                         a_val, nnz_a, b_rowptr, b_col, b_val, nnz_b, p_rowptr, p_col, nnz_p,  \
                         n, out);                                                              \
    else                                                                                       \
      hipLaunchKernelGGL((mp_kernel<1, CC>), dim3(grid), dim3(kMpBlock), 0, s, a_rowptr, a_col, \
                         a_val, nnz_a, b_rowptr, b_col, b_val, nnz_b, p_rowptr, p_col, nnz_p,  \
                         n, out);                                                              \
  } while (0)
  GNN_PER_CHANNELS(C, MP_LAUNCH);
#undef MP_LAUNCH
  return launch_status();
}

extern "C" int gnn_edge_aggregate_f32(const int64_t* rowptr, const int32_t* col,
                                      const float* val, int64_t nnz, int64_t n_rows,
                                      int64_t n_cols, const float* X, int64_t ldx,
                                      int64_t x_stride, float* Y, int64_t ldy, int64_t F, int C,
                                      int skip_diag, void* stream) {
  if (n_rows < 0 || n_cols < 0 || nnz < 0 || x_stride < 0) return GNN_E_ARG;
  const int rc = edge_check_rows(F, C);
  if (rc != GNN_OK) return rc;
  if (n_rows >= kMpDimLimit || n_cols >= kMpDimLimit) return GNN_E_UNSUPPORTED;
  if (ldx < F || ldy < F || (x_stride != 0 && x_stride < n_cols)) return GNN_E_ARG;
  if (n_rows == 0) return GNN_OK;
  if (!rowptr || !Y || (nnz > 0 && (!col || !val || !X))) return GNN_E_ARG;
  if (ldx % 4 || ldy % 4 || !aligned_to(X, 16) || !aligned_to(Y, 16)) return GNN_E_ALIGN;
  const int lg = edge_lanes_log2(F);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned grid = blocks(n_rows << lg, kEaBlock);
#define EA_LAUNCH(CC)                                                                           \
  hipLaunchKernelGGL((ea_kernel<CC>), dim3(grid), dim3(kEaBlock), 0, s, rowptr, col, val, nnz, \
                     n_rows, X, ldx, x_stride, Y, ldy, static_cast<int>(F), lg, skip_diag)
  GNN_PER_CHANNELS(C, EA_LAUNCH);
#undef EA_LAUNCH
  return launch_status();
}

extern "C" int gnn_edge_dot_f32(const int64_t* rowptr, const int32_t* col, int64_t nnz,
                                int64_t n_rows, int64_t n_cols, const float* G, int64_t ldg,
                                const float* X, int64_t ldx, float* dv, int64_t F, int C,
                                int skip_diag, void* stream) {
  if (n_rows < 0 || n_cols < 0 || nnz < 0) return GNN_E_ARG;
  const int rc = edge_check_rows(F, C);
  if (rc != GNN_OK) return rc;
  if (n_rows >= kMpDimLimit || n_cols >= kMpDimLimit) return GNN_E_UNSUPPORTED;
  if (ldx < F || ldg < F) return GNN_E_ARG;
  if (nnz == 0) return GNN_OK;
  if (!rowptr || !col || !G || !X || !dv || n_rows == 0) return GNN_E_ARG;
  if (ldx % 4 || ldg % 4 || !aligned_to(X, 16) || !aligned_to(G, 16)) return GNN_E_ALIGN;
  const int lg = edge_lanes_log2(F);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned grid = blocks(nnz << lg, kEaBlock);
#define ED_LAUNCH(CC)                                                                      \
  hipLaunchKernelGGL((ed_kernel<CC>), dim3(grid), dim3(kEaBlock), 0, s, rowptr, col, nnz, \
                     n_rows, G, ldg, X, ldx, dv, static_cast<int>(F), lg, skip_diag)
  GNN_PER_CHANNELS(C, ED_LAUNCH);
#undef ED_LAUNCH
  return launch_status();
}

extern "C" int gnn_edge_rowsum_f32(const int64_t* rowptr, const int32_t* col, const float* val,
                                   int64_t nnz, int64_t n_rows, int C, int skip_diag, float* y,
                                   void* stream) {
  if (n_rows < 0 || nnz < 0 || C < 1) return GNN_E_ARG;
  if (n_rows >= kMpDimLimit) return GNN_E_UNSUPPORTED;
  if (n_rows == 0) return GNN_OK;
  if (!rowptr || !y || (nnz > 0 && (!col || !val))) return GNN_E_ARG;
  hipLaunchKernelGGL(ers_kernel, dim3(blocks(n_rows * C, 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), rowptr, col, val, nnz, n_rows, C, skip_diag,
                     y);
  return launch_status();
}
