// sup_head.hip -- the head of the supervised training steps on gfx950: the masked mean
// cross entropy of GCN/train_eval.py:45-47, GAT/train_eval.py:73-75 and
// GraphSAGE/train_eval.py:116-117 (nn.CrossEntropyLoss()(output[idx], labels[idx])), the count
// of correct predictions of their accuracy(), and the gradient with respect to the whole
// [N, C] logits.
//
// A row of C logits is held by a group of LPR = the next power of two >= C lanes, lane `sub`
// of the group holding z[r, sub]; a wavefront holds 64 / LPR consecutive rows (or consecutive
// index entries), so with contiguous rows one wave-load covers 64 / LPR * C * 4 contiguous
// bytes (224 of 256 at C = 7). Rows need 4-B alignment only. Every reduction over a row is a
// fixed xor-shuffle tree inside the group. Row arithmetic is in double: m = max_c z,
// lse = m + log sum_c exp(z_c - m), term = lse - z_y, p_c = exp(z_c - lse); each result is
// rounded once.
//
//   gnn_sup_head_count_index / _mask: the selection as an int32 multiplicity count[N]
//     (integer atomic adds over a zeroed buffer; a mask is copied). It is what makes the
//     adjoint a dense, ordered pass instead of a sort plus scatter.
//   gnn_sup_head_fwd_f32: one pass over the selected items (index entries, or the rows with
//     count > 0, or all rows) in a fixed grid: per-block double partials of w term and integer
//     partials of w correct and w valid, then one wavefront adds the partials in a fixed order
//     and writes loss, n_correct and 1 / n_valid. Nothing of size [N, C] is written.
//   gnn_sup_head_bwd_f32: one pass that writes every element of dz exactly once:
//     count[r] (p_c - [c = y_r]) upstream / n_valid recomputed from the logits row, zeros for
//     rows that are not selected or ignored. upstream and 1 / n_valid are read on the device.
// Every index entry is range-checked before it addresses anything (status bit 0) and every
// selected row's label before it addresses a logit (status bit 1); with a status that is not
// zero the loss and the whole gradient are NaN. No floating-point atomics: every result is
// bit-identical from run to run, with duplicates in the index as well.
#include <math.h>

#include "common.hpp"

namespace gnn {

constexpr int kShBlock = 256;
constexpr int kShWaves = kShBlock / kWave;
constexpr int kShMaxBlocks = 2048;
constexpr int kShIters = 4;  // wave iterations per wave before another block is added

// the forward grid: a function of (n, LPR) alone, so the order of the sums is too
static int64_t sh_blocks(int64_t n, int lpr) {
  const int64_t per = static_cast<int64_t>(kShWaves) * (kWave / lpr) * kShIters;
  const int64_t nb = (n + per - 1) / per;
  return nb < 1 ? 1 : nb > kShMaxBlocks ? kShMaxBlocks : nb;
}

__device__ __forceinline__ double sh_shfl_xor_d(double v, int m) {
  return __shfl_xor(v, m, kWave);
}
__device__ __forceinline__ long long sh_shfl_xor_ll(long long v, int m) {
  return __shfl_xor(v, m, kWave);
}

// What a lane group knows about its row after the shuffles (the same in every lane of it).
struct ShRow {
  double lse;  // m + log sum exp(z - m)
  int arg;     // torch.argmax: the first maximum, a NaN counting as the maximum
};

// v: the lane's logit (-inf in the lanes past C, which therefore never win the maximum and
// add exactly 0 to the sum). +inf in the row gives inf - inf = NaN, an all -inf row too, a NaN
// entry makes the sum NaN: torch's results.
template <int LPR>
__device__ __forceinline__ ShRow sh_row(float v, int sub, int C) {
  float m = v;
#pragma unroll
  for (int k = 1; k < LPR; k <<= 1) m = fmaxf(m, shfl_xor_f(m, k));
  double s = sub < C ? exp(static_cast<double>(v) - static_cast<double>(m)) : 0.0;
#pragma unroll
  for (int k = 1; k < LPR; k <<= 1) s += sh_shfl_xor_d(s, k);
  float bv = v;
  int bi = sub;
#pragma unroll
  for (int k = 1; k < LPR; k <<= 1) {
    const float ov = shfl_xor_f(bv, k);
    const int oi = __shfl_xor(bi, k, kWave);
    const bool onan = ov != ov, bnan = bv != bv;
    const bool take = onan ? (!bnan || oi < bi) : (!bnan && (ov > bv || (ov == bv && oi < bi)));
    if (take) {
      bv = ov;
      bi = oi;
    }
  }
  return ShRow{static_cast<double>(m) + log(s), bi};
}

__global__ __launch_bounds__(kShBlock) void sup_count_index_kernel(
    const int64_t* __restrict__ index, int64_t n, int64_t N, int32_t* __restrict__ count,
    uint32_t* __restrict__ status) {
  const int64_t step = static_cast<int64_t>(gridDim.x) * kShBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kShBlock + threadIdx.x; i < n; i += step) {
    int64_t r = index[i];
    if (r < 0) r += N;
    if (r < 0 || r >= N)
      atomicOr(status, 1u);
    else
      atomicAdd(count + r, 1);
  }
}

__global__ __launch_bounds__(kShBlock) void sup_count_mask_kernel(
    const uint8_t* __restrict__ mask, int64_t N, int32_t* __restrict__ count) {
  const int64_t step = static_cast<int64_t>(gridDim.x) * kShBlock;
  for (int64_t r = static_cast<int64_t>(blockIdx.x) * kShBlock + threadIdx.x; r < N; r += step)
    count[r] = mask[r] != 0;
}

// Item i is row index[i] once (index given), or row i count[i] times (count given), or row i
// once. part[b]: block b's sum of w term; ipart[2 b], ipart[2 b + 1]: of w correct, w valid.
template <int LPR>
__global__ __launch_bounds__(kShBlock) void sup_head_fwd_kernel(
    const float* __restrict__ z, int64_t ldz, const int64_t* __restrict__ labels,
    const int64_t* __restrict__ index, const int32_t* __restrict__ count, int64_t n, int64_t N,
    int C, int64_t ignore, uint32_t* __restrict__ status, double* __restrict__ part,
    long long* __restrict__ ipart) {
  constexpr int G = kWave / LPR;
  __shared__ double wsum[kShWaves];
  __shared__ long long wcnt[2][kShWaves];
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane & (LPR - 1), grp = lane / LPR;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kShWaves + (threadIdx.x >> 6);
  const int64_t step = static_cast<int64_t>(gridDim.x) * kShWaves * G;
  double acc = 0.0;
  long long ncorrect = 0, nvalid = 0;
  uint32_t bad = 0;
  for (int64_t i0 = wave * G; i0 < n; i0 += step) {  // the same trip count in every lane
    const int64_t i = i0 + grp;
    int64_t r = 0;
    int32_t w = 0;
    if (i < n) {
      if (index) {
        r = index[i];
        if (r < 0) r += N;
        if (r < 0 || r >= N)
          bad |= 1u;
        else
          w = 1;
      } else {
        r = i;
        w = count ? count[i] : 1;
      }
    }
    int64_t y = ignore;
    if (w > 0) y = labels[r];
    bool use = w > 0 && y != ignore;
    if (use && (y < 0 || y >= C)) {
      bad |= 2u;
      use = false;
    }
    if (!__any(use)) continue;
    float v = -INFINITY;
    if (use && sub < C) v = z[r * ldz + sub];
    const ShRow row = sh_row<LPR>(v, sub, C);
    const float zy = __shfl(v, (lane & ~(LPR - 1)) + (use ? static_cast<int>(y) : 0), kWave);
    if (use && sub == 0) {
      acc += static_cast<double>(w) * (row.lse - static_cast<double>(zy));
      ncorrect += row.arg == y ? w : 0;
      nvalid += w;
    }
  }
  if (bad) atomicOr(status, bad);
#pragma unroll
  for (int k = 1; k < kWave; k <<= 1) {
    acc += sh_shfl_xor_d(acc, k);
    ncorrect += sh_shfl_xor_ll(ncorrect, k);
    nvalid += sh_shfl_xor_ll(nvalid, k);
  }
  if (lane == 0) {
    wsum[threadIdx.x >> 6] = acc;
    wcnt[0][threadIdx.x >> 6] = ncorrect;
    wcnt[1][threadIdx.x >> 6] = nvalid;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = wsum[0];
    long long c0 = wcnt[0][0], c1 = wcnt[1][0];
#pragma unroll
    for (int k = 1; k < kShWaves; ++k) {
      t += wsum[k];
      c0 += wcnt[0][k];
      c1 += wcnt[1][k];
    }
    part[blockIdx.x] = t;
    ipart[2 * blockIdx.x] = c0;
    ipart[2 * blockIdx.x + 1] = c1;
  }
}

// one wavefront: lane l adds partials l, l + 64, ... in that order, then a fixed xor tree
__global__ __launch_bounds__(kWave) void sup_head_finish_kernel(
    const double* __restrict__ part, const long long* __restrict__ ipart, int nb,
    const uint32_t* __restrict__ status, float* __restrict__ loss,
    int64_t* __restrict__ n_correct, double* __restrict__ inv_valid) {
  double acc = 0.0;
  long long c0 = 0, c1 = 0;
  for (int i = threadIdx.x; i < nb; i += kWave) {
    acc += part[i];
    c0 += ipart[2 * i];
    c1 += ipart[2 * i + 1];
  }
#pragma unroll
  for (int k = 1; k < kWave; k <<= 1) {
    acc += sh_shfl_xor_d(acc, k);
    c0 += sh_shfl_xor_ll(c0, k);
    c1 += sh_shfl_xor_ll(c1, k);
  }
  if (threadIdx.x == 0) {
    const double nv = static_cast<double>(c1);
    // no valid row: 0 / 0 = NaN, torch's mean of nothing
    loss[0] = status[0] ? NAN : static_cast<float>(acc / nv);
    if (n_correct) n_correct[0] = c0;
    inv_valid[0] = 1.0 / nv;
  }
}

// A wavefront takes 64 consecutive rows at a time, one row per lane for the multiplicity and
// the label. Rows that are not evaluated (count 0, an ignored label) get their zeros straight
// away, 64 / LPR rows per store; the rows that are evaluated are ranked by a ballot, their
// (row, count, label) moved to lanes 0 .. n_use - 1 by one ds_permute each, and the lane groups
// then take them 64 / LPR at a time: a selection of every 10th row costs one round of row
// arithmetic per 64 rows, not one per 64 / LPR.
template <int LPR>
__global__ __launch_bounds__(kShBlock) void sup_head_bwd_kernel(
    const float* __restrict__ z, int64_t ldz, const int64_t* __restrict__ labels,
    const int32_t* __restrict__ count, int64_t N, int C, int64_t ignore,
    const float* __restrict__ upstream, const double* __restrict__ inv_valid,
    const uint32_t* __restrict__ status, float* __restrict__ dz, int64_t lddz) {
  constexpr int G = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane & (LPR - 1), grp = lane / LPR;
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kShWaves + (threadIdx.x >> 6);
  const int64_t step = static_cast<int64_t>(gridDim.x) * kShBlock;
  const bool poisoned = status[0] != 0;
  const double scale = static_cast<double>(upstream[0]) * inv_valid[0];
  for (int64_t r0 = wave * kWave; r0 < N; r0 += step) {
    const int64_t rl = r0 + lane;
    int32_t w = 0;
    if (rl < N && !poisoned) w = count ? count[rl] : 1;
    int64_t y = ignore;
    if (w > 0) y = labels[rl];
    bool use = w > 0 && y != ignore;
    const bool badlabel = use && (y < 0 || y >= C);
    if (badlabel) use = false;
    const uint64_t mask = __ballot(use);
    const uint64_t nanmask = poisoned ? ~0ull : __ballot(badlabel);
    if (mask != ~0ull) {
      for (int j = grp; j < kWave; j += G) {
        const int64_t r = r0 + j;
        if (r < N && sub < C && !((mask >> j) & 1))
          dz[r * lddz + sub] = ((nanmask >> j) & 1) ? NAN : 0.f;
      }
    }
    const int n_use = __popcll(mask);
    if (n_use == 0) continue;
    // a permutation of the lanes: the evaluated rows first, in row order
    const int rank = __popcll(mask & ((1ull << lane) - 1));
    const int dest = (use ? rank : n_use + lane - rank) << 2;
    const int pj = __builtin_amdgcn_ds_permute(dest, lane);
    const int pw = __builtin_amdgcn_ds_permute(dest, w);
    const int py = __builtin_amdgcn_ds_permute(dest, static_cast<int>(y));
    for (int q0 = 0; q0 < n_use; q0 += G) {
      const int q = q0 + grp;  // < 64
      const bool on = q < n_use;
      const int64_t r = r0 + __shfl(pj, q, kWave);
      const int wq = __shfl(pw, q, kWave), yq = __shfl(py, q, kWave);
      float v = -INFINITY;
      if (on && sub < C) v = z[r * ldz + sub];
      const ShRow row = sh_row<LPR>(v, sub, C);
      const double p = exp(static_cast<double>(v) - row.lse);
      const double g = static_cast<double>(wq) * (p - (sub == yq ? 1.0 : 0.0)) * scale;
      if (on && sub < C) dz[r * lddz + sub] = static_cast<float>(g);
    }
  }
}

static int sh_lpr(int64_t C) { return C <= 2 ? 2 : next_pow2_le64(C); }

static unsigned sh_flat_blocks(int64_t n) {
  const int64_t nb = (n + kShBlock - 1) / kShBlock;
  return static_cast<unsigned>(nb < 1 ? 1 : nb > kShMaxBlocks ? kShMaxBlocks : nb);
}

template <int LPR>
static void launch_sup_fwd(const float* z, int64_t ldz, const int64_t* labels,
                           const int64_t* index, const int32_t* count, int64_t n, int64_t N,
                           int C, int64_t ignore, uint32_t* status, double* part,
                           long long* ipart, int nb, hipStream_t s) {
  hipLaunchKernelGGL(sup_head_fwd_kernel<LPR>, dim3(nb), dim3(kShBlock), 0, s, z, ldz, labels,
                     index, count, n, N, C, ignore, status, part, ipart);
}

template <int LPR>
static void launch_sup_bwd(const float* z, int64_t ldz, const int64_t* labels,
                           const int32_t* count, int64_t N, int C, int64_t ignore,
                           const float* upstream, const double* inv_valid,
                           const uint32_t* status, float* dz, int64_t lddz, hipStream_t s) {
  // 64 rows per wavefront up to the cap, a grid stride past it
  int64_t nb = (N + kShBlock - 1) / kShBlock;
  if (nb > 4 * kShMaxBlocks) nb = 4 * kShMaxBlocks;
  hipLaunchKernelGGL(sup_head_bwd_kernel<LPR>, dim3(static_cast<unsigned>(nb)), dim3(kShBlock),
                     0, s, z, ldz, labels, count, N, C, ignore, upstream, inv_valid, status, dz,
                     lddz);
}

}  // namespace gnn

using namespace gnn;

extern "C" int gnn_sup_head_supported(int64_t C) { return C >= 2 && C <= 64; }

extern "C" int64_t gnn_sup_head_workspace_bytes(int64_t n) {
  if (n < 0) return GNN_E_ARG;
  // the widest lane group (one row per wavefront) has the most blocks: 24 B per block
  return (sh_blocks(n, kWave) * 24 + 255) / 256 * 256;
}

extern "C" int gnn_sup_head_count_index(const int64_t* index, int64_t n, int64_t N,
                                        int32_t* count, uint32_t* status, void* stream) {
  if (n < 0 || N < 0) return GNN_E_ARG;
  if (N > 0 && (!count || !status)) return GNN_E_ARG;
  if (N > 0 && n > 0 && !index) return GNN_E_ARG;
  if (N > INT64_MAX / 8 || n > 0x7fffffffLL) return GNN_E_UNSUPPORTED;  // a count fits int32
  if (!aligned_to(index, 8) || !aligned_to(count, 4) || !aligned_to(status, 4))
    return GNN_E_ALIGN;
  if (N == 0) return GNN_OK;  // nothing to count into
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(count, 0, static_cast<size_t>(N) * sizeof(int32_t), s);
  if (e != hipSuccess) return static_cast<int>(e);
  if (n > 0)
    hipLaunchKernelGGL(sup_count_index_kernel, dim3(sh_flat_blocks(n)), dim3(kShBlock), 0, s,
                       index, n, N, count, status);
  return launch_status();
}

extern "C" int gnn_sup_head_count_mask(const uint8_t* mask, int64_t N, int32_t* count,
                                       void* stream) {
  if (N < 0) return GNN_E_ARG;
  if (N > 0 && (!mask || !count)) return GNN_E_ARG;
  if (N > INT64_MAX / 8) return GNN_E_UNSUPPORTED;
  if (!aligned_to(count, 4)) return GNN_E_ALIGN;
  if (N == 0) return GNN_OK;
  hipLaunchKernelGGL(sup_count_mask_kernel, dim3(sh_flat_blocks(N)), dim3(kShBlock), 0,
                     static_cast<hipStream_t>(stream), mask, N, count);
  return launch_status();
}

extern "C" int gnn_sup_head_fwd_f32(const float* z, int64_t ldz, const int64_t* labels,
                                    const int64_t* index, const int32_t* count, int64_t n,
                                    int64_t N, int64_t C, int64_t ignore_index, float* loss,
                                    int64_t* n_correct, double* inv_valid, uint32_t* status,
                                    void* ws, int64_t ws_bytes, void* stream) {
  if (n < 0 || N < 0 || C < 0) return GNN_E_ARG;
  if (!gnn_sup_head_supported(C)) return GNN_E_UNSUPPORTED;
  if (ldz < C) return GNN_E_ARG;
  if (index ? count != nullptr : n != N) return GNN_E_ARG;  // one description of the selection
  if (n > 0 && (!z || !labels || !loss || !inv_valid || !status || !ws)) return GNN_E_ARG;
  if (N > INT64_MAX / 16 / ldz) return GNN_E_UNSUPPORTED;  // r ldz stays inside int64
  if (n > 0 && ws_bytes < gnn_sup_head_workspace_bytes(n)) return GNN_E_ARG;
  if (!aligned_to(z, 4) || !aligned_to(labels, 8) || !aligned_to(index, 8) ||
      !aligned_to(count, 4) || !aligned_to(loss, 4) || !aligned_to(n_correct, 8) ||
      !aligned_to(inv_valid, 8) || !aligned_to(status, 4) || !aligned_to(ws, 8))
    return GNN_E_ALIGN;
  if (n == 0) return GNN_OK;  // the mean of nothing is the caller's NaN
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int lpr = sh_lpr(C);
  const int nb = static_cast<int>(sh_blocks(n, lpr));
  const int64_t slots = sh_blocks(n, kWave);
  double* part = static_cast<double*>(ws);
  long long* ipart = reinterpret_cast<long long*>(part + slots);
  const int c = static_cast<int>(C);
#define SH_FWD(L)                                                                            \
  case L:                                                                                    \
    launch_sup_fwd<L>(z, ldz, labels, index, count, n, N, c, ignore_index, status, part,     \
                      ipart, nb, s);                                                         \
    break
  switch (lpr) {
    SH_FWD(2);
    SH_FWD(4);
    SH_FWD(8);
    SH_FWD(16);
    SH_FWD(32);
    SH_FWD(64);
  }
#undef SH_FWD
  hipLaunchKernelGGL(sup_head_finish_kernel, dim3(1), dim3(kWave), 0, s, part, ipart, nb, status,
                     loss, n_correct, inv_valid);
  return launch_status();
}

extern "C" int gnn_sup_head_bwd_f32(const float* z, int64_t ldz, const int64_t* labels,
                                    const int32_t* count, int64_t N, int64_t C,
                                    int64_t ignore_index, const float* upstream,
                                    const double* inv_valid, const uint32_t* status, float* dz,
                                    int64_t lddz, void* stream) {
  if (N < 0 || C < 0) return GNN_E_ARG;
  if (!gnn_sup_head_supported(C)) return GNN_E_UNSUPPORTED;
  if (ldz < C || lddz < C) return GNN_E_ARG;
  if (N > 0 && (!z || !labels || !upstream || !inv_valid || !status || !dz)) return GNN_E_ARG;
  if (N > INT64_MAX / 16 / ldz || N > INT64_MAX / 16 / lddz) return GNN_E_UNSUPPORTED;
  if (!aligned_to(z, 4) || !aligned_to(labels, 8) || !aligned_to(count, 4) ||
      !aligned_to(upstream, 4) || !aligned_to(inv_valid, 8) || !aligned_to(status, 4) ||
      !aligned_to(dz, 4))
    return GNN_E_ALIGN;
  if (N == 0) return GNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int c = static_cast<int>(C);
#define SH_BWD(L)                                                                            \
  case L:                                                                                    \
    launch_sup_bwd<L>(z, ldz, labels, count, N, c, ignore_index, upstream, inv_valid,        \
                      status, dz, lddz, s);                                                  \
    break
  switch (sh_lpr(C)) {
    SH_BWD(2);
    SH_BWD(4);
    SH_BWD(8);
    SH_BWD(16);
    SH_BWD(32);
    SH_BWD(64);
  }
#undef SH_BWD
  return launch_status();
}
