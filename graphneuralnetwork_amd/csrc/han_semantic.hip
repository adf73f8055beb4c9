// han_semantic.hip -- HAN's metapath-level ("semantic") attention on gfx950
// (HAN/models/SemanticAttention.py:15-20):
//   w = mean_n(w2 . tanh(W1 z[n, m] + b1)),  beta = softmax_m(w),  out[n] = sum_m beta[m] z[n, m]
// and its adjoint. z[n, m, :] lives at z + n ld_n + m ld_m (D floats, 16-B aligned); the rows
// r = n M + m of the [N M, D] view go through the matrix cores in tiles of 64 on a persistent
// grid with W1 [S = 128, D] resident in registers. Nothing of size [N M, S] is ever written.
//
// Arithmetic: v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation) for every product.
// tanh(x) = 1 - 2 / (1 + exp(2x)) on the hardware exponential and reciprocal: exp -> inf gives
// 1, exp -> 0 gives -1, NaN stays NaN; no clamp. Every sum has an order fixed by the shapes
// (no floating-point atomics): results are bit-identical from run to run.
//
//   han_scores_kernel    GEMM1 per tile (4 waves x 32 of the 128 hidden columns), epilogue
//                        s_r = w2 . tanh(.) in registers, the four waves' pieces added in wave
//                        order through LDS, per-metapath sums kept in double by the 64 row
//                        threads; one partial per (workgroup, m).
//   han_finish_kernel    one wavefront: partials in workgroup order (double), w = sum / N,
//                        beta = softmax(w) with the maximum subtracted.
//   han_combine_kernel   out[n] = sum_m beta[m] z[n, m], m ascending, 16-B loads and stores.
//   han_dbeta_kernel     dbeta[m] = sum_n g[n] . z[n, m]: one streaming pass, double partials.
//   han_coef_kernel      one wavefront: dw = beta (dbeta - sum_k beta_k dbeta_k), c = dw / N.
//   han_dz_kernel        GEMM1 again, q = c[m] w2 (1 - t^2) through LDS (over the z tile, which
//                        is dead by then), GEMM2 dz = beta[m] g[n] + q W1 with W1^T resident.
//   han_dparam_kernel    GEMM1 transposed (rows on the accumulator registers), so q feeds the
//                        third MFMA dW1 += q^T z as its A operand straight from the
//                        accumulators; dW1 [S, D], db1 and dw2 stay in registers over all of a
//                        workgroup's tiles, one partial per workgroup, summed in a fixed
//                        order (double) by han_param_reduce_kernel.
#include <math.h>

#include "common.hpp"

extern "C" int gnn_han_semantic_supported(int64_t D, int64_t S, int64_t M);

namespace gnn {

constexpr int kHsS = 128;        // hidden width of the projection
constexpr int kHsTR = 64;        // rows per tile
constexpr int kHsBlock = 256;    // 4 waves
constexpr int kHsMaxM = 8;
constexpr int kHsGrid = 512;     // persistent grid of the scores / dz kernels (2 per CU)
constexpr int kHsParamGrid = 256;  // of the parameter-gradient kernel: one partial each
constexpr int kHsFlatGrid = 512;   // dbeta pass: one partial each
using hs4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float han_tanh(float x) {
  const float e = __expf(2.f * x);
  return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + e);
}

__device__ __forceinline__ double hs_shfl_xor_d(double v, int m) { return __shfl_xor(v, m, kWave); }

static int64_t hs_tiles(int64_t rows) { return (rows + kHsTR - 1) / kHsTR; }
static int hs_grid(int64_t rows, int cap) {
  const int64_t t = hs_tiles(rows);
  return static_cast<int>(t < 1 ? 1 : t > cap ? cap : t);
}
static int hs_flat_grid(int64_t N, int64_t D) {
  const int64_t per = static_cast<int64_t>(kHsBlock) * 4;
  const int64_t nb = (N * (D / 4) + per - 1) / per;
  return static_cast<int>(nb < 1 ? 1 : nb > kHsFlatGrid ? kHsFlatGrid : nb);
}

// The tile machinery shared by the three MFMA kernels: a tile is 64 rows of D floats, every
// thread moving NV = D / 16 float4s of it, staged in LDS in the TileLds<D> layout.
template <int D>
struct HsTile {
  static constexpr int KS = D / 4;  // k-steps of GEMM1; lane quarter kq owns d in [kq KS, kq KS + KS)
  static constexpr int LDA = 4 * TileLds<D>::L4;
  static constexpr int NV = kHsTR * (D / 4) / kHsBlock;
  static_assert(NV * kHsBlock == kHsTR * (D / 4), "every thread stages NV float4s");

  // rows past the end (and whole tiles past the last) read nothing and give zeros
  static __device__ __forceinline__ void fetch(float4 (&p)[NV], const float* __restrict__ z,
                                               int64_t ld_n, int64_t ld_m, int64_t rows, int M,
                                               int64_t g) {
    const int64_t row0 = g * kHsTR;
    const int64_t n0 = row0 / M;
    const int m0 = static_cast<int>(row0 - n0 * M);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int e = v * kHsBlock + static_cast<int>(threadIdx.x);
      const int rr = e / (D / 4), c4 = e - rr * (D / 4);
      p[v] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row0 + rr < rows) {
        const int t = m0 + rr, dn = t / M, m = t - dn * M;
        p[v] = *reinterpret_cast<const float4*>(z + (n0 + dn) * ld_n + m * ld_m + 4 * c4);
      }
    }
  }
  static __device__ __forceinline__ void stage(float* __restrict__ xt, const float4 (&p)[NV]) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int e = v * kHsBlock + static_cast<int>(threadIdx.x);
      const int rr = e / (D / 4), c4 = e - rr * (D / 4);
      *reinterpret_cast<float4*>(xt + rr * LDA + 4 * (c4 ^ TileLds<D>::swz(rr))) = p[v];
    }
  }
  // W1[(2 wv + cb) 16 + r][kq KS + s]: this lane's share of the wave's 32 hidden columns
  static __device__ __forceinline__ void load_w1(float (&wa)[2][KS], const float* __restrict__ w1,
                                                 int wv, int kq, int r) {
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const float* wr = w1 + ((wv * 2 + cb) * 16 + r) * D + kq * KS;
#pragma unroll
      for (int v = 0; v < KS / 4; ++v) {
        const float4 t = *reinterpret_cast<const float4*>(wr + 4 * v);
        wa[cb][4 * v] = t.x;
        wa[cb][4 * v + 1] = t.y;
        wa[cb][4 * v + 2] = t.z;
        wa[cb][4 * v + 3] = t.w;
      }
    }
  }
  // tile row 16 j + r, this lane quarter's KS values
  static __device__ __forceinline__ void load_x(float (&xb)[KS], const float* __restrict__ xt,
                                                int j, int kq, int r) {
    const int rr = j * 16 + r;
    const float* xr = xt + rr * LDA;
#pragma unroll
    for (int v = 0; v < KS / 4; ++v) {
      const int c4 = kq * (KS / 4) + v;
      const float4 t = *reinterpret_cast<const float4*>(xr + 4 * (c4 ^ TileLds<D>::swz(rr)));
      xb[4 * v] = t.x;
      xb[4 * v + 1] = t.y;
      xb[4 * v + 2] = t.z;
      xb[4 * v + 3] = t.w;
    }
  }
  static __device__ __forceinline__ float elem(const float* __restrict__ xt, int rr, int d) {
    return xt[rr * LDA + 4 * ((d >> 2) ^ TileLds<D>::swz(rr)) + (d & 3)];
  }
};

// ---------------------------------------------------------------------------------------
// scores: part[8 b + m] = workgroup b's sum over its rows of metapath m of w2 . tanh(W1 z + b1)
template <int D>
__global__ __launch_bounds__(kHsBlock) void han_scores_kernel(
    const float* __restrict__ z, int64_t ld_n, int64_t ld_m, int64_t rows, int M,
    const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
    double* __restrict__ part) {
  using T = HsTile<D>;
  constexpr int KS = T::KS;
  __shared__ float xt[kHsTR * T::LDA];
  __shared__ float ps[4][kHsTR];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int kq = lane >> 4, r = lane & 15;
  float wa[2][KS];
  T::load_w1(wa, w1, wv, kq, r);
  float b1v[2][4], w2v[2][4];  // hidden columns (2 wv + cb) 16 + 4 kq + i
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      b1v[cb][i] = b1[(wv * 2 + cb) * 16 + 4 * kq + i];
      w2v[cb][i] = w2[(wv * 2 + cb) * 16 + 4 * kq + i];
    }
  double am[kHsMaxM];
#pragma unroll
  for (int k = 0; k < kHsMaxM; ++k) am[k] = 0.0;
  const int64_t tiles = (rows + kHsTR - 1) / kHsTR;
  float4 pre[T::NV];
  T::fetch(pre, z, ld_n, ld_m, rows, M, blockIdx.x);
  for (int64_t g = blockIdx.x; g < tiles; g += gridDim.x) {
    __syncthreads();  // the previous tile's xt and ps are free
    T::stage(xt, pre);
    __syncthreads();
    T::fetch(pre, z, ld_n, ld_m, rows, M, g + gridDim.x);
#pragma unroll
    for (int j = 0; j < kHsTR / 16; ++j) {
      float xb[KS];
      T::load_x(xb, xt, j, kq, r);
      hs4 acc[2] = {hs4{0.f, 0.f, 0.f, 0.f}, hs4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
          acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[cb][s], xb[s], acc[cb], 0, 0, 0);
      // acc[cb][i] = (W1 z)[row 16 j + r][column (2 wv + cb) 16 + 4 kq + i]
      float p = 0.f;
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int i = 0; i < 4; ++i) p = fmaf(w2v[cb][i], han_tanh(acc[cb][i] + b1v[cb][i]), p);
      p += __shfl_xor(p, 16, kWave);
      p += __shfl_xor(p, 32, kWave);
      if (kq == 0) ps[wv][j * 16 + r] = p;
    }
    __syncthreads();
    if (threadIdx.x < kHsTR) {
      const int t = static_cast<int>(threadIdx.x);
      const int64_t R = g * kHsTR + t;
      const float s = ((ps[0][t] + ps[1][t]) + ps[2][t]) + ps[3][t];
      if (R < rows) {
        const int m = static_cast<int>(R % M);
#pragma unroll
        for (int k = 0; k < kHsMaxM; ++k) am[k] += k == m ? static_cast<double>(s) : 0.0;
      }
    }
  }
  if (threadIdx.x < kWave) {  // wave 0 holds the sums
#pragma unroll
    for (int k = 0; k < kHsMaxM; ++k) {
#pragma unroll
      for (int x = 1; x < kWave; x <<= 1) am[k] += hs_shfl_xor_d(am[k], x);
      if (lane == 0) part[static_cast<int64_t>(blockIdx.x) * kHsMaxM + k] = am[k];
    }
  }
}

// one wavefront: lane l adds partials l, l + 64, ... in that order, then a fixed xor tree
__device__ __forceinline__ void hs_sum_partials(const double* __restrict__ part, int nb,
                                                double (&acc)[kHsMaxM]) {
#pragma unroll
  for (int k = 0; k < kHsMaxM; ++k) acc[k] = 0.0;
  for (int i = threadIdx.x; i < nb; i += kWave)
#pragma unroll
    for (int k = 0; k < kHsMaxM; ++k) acc[k] += part[static_cast<int64_t>(i) * kHsMaxM + k];
#pragma unroll
  for (int k = 0; k < kHsMaxM; ++k)
#pragma unroll
    for (int x = 1; x < kWave; x <<= 1) acc[k] += hs_shfl_xor_d(acc[k], x);
}

__global__ __launch_bounds__(kWave) void han_finish_kernel(const double* __restrict__ part, int nb,
                                                           int M, int64_t N,
                                                           float* __restrict__ w,
                                                           float* __restrict__ beta) {
  double acc[kHsMaxM];
  hs_sum_partials(part, nb, acc);
  if (threadIdx.x != 0) return;
  // torch.softmax: the maximum subtracted; a NaN score makes every beta NaN
  double mx = -INFINITY, den = 0.0, e[kHsMaxM];
#pragma unroll
  for (int k = 0; k < kHsMaxM; ++k) {
    acc[k] /= static_cast<double>(N);
    if (k < M) mx = fmax(mx, acc[k]);
  }
#pragma unroll
  for (int k = 0; k < kHsMaxM; ++k) {
    e[k] = k < M ? exp(acc[k] - mx) : 0.0;
    den += e[k];
  }
#pragma unroll
  for (int k = 0; k < kHsMaxM; ++k)
    if (k < M) {
      if (w) w[k] = static_cast<float>(acc[k]);
      beta[k] = static_cast<float>(e[k] / den);
    }
}

__global__ __launch_bounds__(kHsBlock) void han_combine_kernel(
    const float* __restrict__ z, int64_t ld_n, int64_t ld_m, int64_t N, int M, int D4,
    const float* __restrict__ beta, float* __restrict__ out, int64_t ldo) {
  float bv[kHsMaxM];
#pragma unroll
  for (int k = 0; k < kHsMaxM; ++k) bv[k] = k < M ? beta[k] : 0.f;
  const int64_t total = N * D4, step = static_cast<int64_t>(gridDim.x) * kHsBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kHsBlock + threadIdx.x; i < total;
       i += step) {
    const int64_t n = i / D4;
    const int c4 = static_cast<int>(i - n * D4);
    const float* zr = z + n * ld_n + 4 * c4;
    float4 a = *reinterpret_cast<const float4*>(zr);
    a.x *= bv[0];
    a.y *= bv[0];
    a.z *= bv[0];
    a.w *= bv[0];
#pragma unroll
    for (int k = 1; k < kHsMaxM; ++k)
      if (k < M) {
        const float4 t = *reinterpret_cast<const float4*>(zr + k * ld_m);
        a.x = fmaf(bv[k], t.x, a.x);
        a.y = fmaf(bv[k], t.y, a.y);
        a.z = fmaf(bv[k], t.z, a.z);
        a.w = fmaf(bv[k], t.w, a.w);
      }
    *reinterpret_cast<float4*>(out + n * ldo + 4 * c4) = a;
  }
}

// ---------------------------------------------------------------------------------------
// adjoint (a): part[8 b + m] = workgroup b's share of sum_n g[n] . z[n, m]
__global__ __launch_bounds__(kHsBlock) void han_dbeta_kernel(
    const float* __restrict__ g, int64_t ldg, const float* __restrict__ z, int64_t ld_n,
    int64_t ld_m, int64_t N, int M, int D4, double* __restrict__ part) {
  __shared__ double ws[kHsBlock / kWave][kHsMaxM];
  double acc[kHsMaxM];
#pragma unroll
  for (int k = 0; k < kHsMaxM; ++k) acc[k] = 0.0;
  const int64_t total = N * D4, step = static_cast<int64_t>(gridDim.x) * kHsBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kHsBlock + threadIdx.x; i < total;
       i += step) {
    const int64_t n = i / D4;
    const int c4 = static_cast<int>(i - n * D4);
    const float4 gv = *reinterpret_cast<const float4*>(g + n * ldg + 4 * c4);
    const float* zr = z + n * ld_n + 4 * c4;
#pragma unroll
    for (int k = 0; k < kHsMaxM; ++k)
      if (k < M) {
        const float4 t = *reinterpret_cast<const float4*>(zr + k * ld_m);
        acc[k] += static_cast<double>(fmaf(gv.x, t.x, fmaf(gv.y, t.y, fmaf(gv.z, t.z, gv.w * t.w))));
      }
  }
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kHsMaxM; ++k) {
#pragma unroll
    for (int x = 1; x < kWave; x <<= 1) acc[k] += hs_shfl_xor_d(acc[k], x);
    if (lane == 0) ws[wv][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < kHsMaxM) {
    double t = ws[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < kHsBlock / kWave; ++q) t += ws[q][threadIdx.x];
    part[static_cast<int64_t>(blockIdx.x) * kHsMaxM + threadIdx.x] = t;
  }
}

// adjoint (b): coef[m] = beta[m] (dbeta[m] - sum_k beta[k] dbeta[k]) / N, zero for m >= M
__global__ __launch_bounds__(kWave) void han_coef_kernel(const double* __restrict__ part, int nb,
                                                         int M, int64_t N,
                                                         const float* __restrict__ beta,
                                                         float* __restrict__ coef) {
  double acc[kHsMaxM];
  hs_sum_partials(part, nb, acc);
  if (threadIdx.x != 0) return;
  double dot = 0.0, b[kHsMaxM];
#pragma unroll
  for (int k = 0; k < kHsMaxM; ++k) {
    b[k] = k < M ? static_cast<double>(beta[k]) : 0.0;
    if (k < M) dot += b[k] * acc[k];
  }
#pragma unroll
  for (int k = 0; k < kHsMaxM; ++k)
    coef[k] = k < M ? static_cast<float>(b[k] * (acc[k] - dot) / static_cast<double>(N)) : 0.f;
}

// per-row constants of a tile: coefficient c[m] and beta[m] of the row's metapath, 0 past the end
__device__ __forceinline__ void hs_row_consts(float* __restrict__ cm, float* __restrict__ bm,
                                              const float* __restrict__ coef,
                                              const float* __restrict__ beta, int64_t g,
                                              int64_t rows, int M) {
  if (threadIdx.x < kHsTR) {
    const int64_t R = g * kHsTR + threadIdx.x;
    const bool on = R < rows;
    const int m = on ? static_cast<int>(R % M) : 0;
    cm[threadIdx.x] = on ? coef[m] : 0.f;
    if (bm) bm[threadIdx.x] = on ? beta[m] : 0.f;
  }
}

// adjoint (c), input side: dz[n, m] = beta[m] g[n] + q W1, q = c[m] w2 (1 - tanh^2(W1 z + b1)).
// GEMM2 splits the tile over the waves by output column block where D has at least four
// (NB = D / 16 blocks; every wave all four 16-row blocks), else by row block as well.
template <int D>
__global__ __launch_bounds__(kHsBlock) void han_dz_kernel(
    const float* __restrict__ z, int64_t ld_n, int64_t ld_m, int64_t rows, int M,
    const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ coef, const float* __restrict__ beta, const float* __restrict__ gy,
    int64_t ldg, float* __restrict__ dz, int64_t ldd_n, int64_t ldd_m) {
  using T = HsTile<D>;
  constexpr int KS = T::KS;
  constexpr int NB = D / 16;                 // output column blocks
  constexpr int CBD = NB >= 4 ? NB / 4 : 1;  // ... per wave
  constexpr int WD = NB >= 4 ? 4 : NB;       // waves across the column blocks
  constexpr int JR = 4 / (4 / WD);           // row blocks per wave = WD
  constexpr int LQ = kHsS + 4;               // q tile pitch (floats)
  constexpr int kLds = kHsTR * (T::LDA > LQ ? T::LDA : LQ);
  __shared__ float xt[kLds];  // the z tile, then the q tile
  __shared__ float cm[kHsTR], bm[kHsTR];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int kq = lane >> 4, r = lane & 15;
  float wa[2][KS];
  T::load_w1(wa, w1, wv, kq, r);
  float b1v[2][4], w2v[2][4];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      b1v[cb][i] = b1[(wv * 2 + cb) * 16 + 4 * kq + i];
      w2v[cb][i] = w2[(wv * 2 + cb) * 16 + 4 * kq + i];
    }
  // GEMM2's A operand: W1[s = 32 kq + st][d = blk 16 + r] for this wave's column blocks
  const int db0 = (wv % WD) * CBD, j0 = (wv / WD) * JR;
  float wt[CBD][kHsS / 4];
#pragma unroll
  for (int c = 0; c < CBD; ++c)
#pragma unroll
    for (int st = 0; st < kHsS / 4; ++st)
      wt[c][st] = w1[(kq * (kHsS / 4) + st) * D + (db0 + c) * 16 + r];
  const int64_t tiles = (rows + kHsTR - 1) / kHsTR;
  float4 pre[T::NV];
  T::fetch(pre, z, ld_n, ld_m, rows, M, blockIdx.x);
  for (int64_t g = blockIdx.x; g < tiles; g += gridDim.x) {
    __syncthreads();  // the previous tile's q and row constants are free
    T::stage(xt, pre);
    hs_row_consts(cm, bm, coef, beta, g, rows, M);
    __syncthreads();
    T::fetch(pre, z, ld_n, ld_m, rows, M, g + gridDim.x);
    hs4 qv[kHsTR / 16][2];
#pragma unroll
    for (int j = 0; j < kHsTR / 16; ++j) {
      float xb[KS];
      T::load_x(xb, xt, j, kq, r);
      hs4 acc[2] = {hs4{0.f, 0.f, 0.f, 0.f}, hs4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
          acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[cb][s], xb[s], acc[cb], 0, 0, 0);
      const float c = cm[j * 16 + r];
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float t = han_tanh(acc[cb][i] + b1v[cb][i]);
          qv[j][cb][i] = c * w2v[cb][i] * (1.f - t * t);
        }
    }
    __syncthreads();  // every wave has read the z tile: q goes over it
#pragma unroll
    for (int j = 0; j < kHsTR / 16; ++j)
#pragma unroll
      for (int cb = 0; cb < 2; ++cb)
        *reinterpret_cast<hs4*>(xt + (j * 16 + r) * LQ + (wv * 2 + cb) * 16 + 4 * kq) = qv[j][cb];
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < JR; ++jj) {
      const int j = j0 + jj;
      const float* qr = xt + (j * 16 + r) * LQ + kq * (kHsS / 4);
      hs4 acc2[CBD];
#pragma unroll
      for (int c = 0; c < CBD; ++c) acc2[c] = hs4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int v = 0; v < kHsS / 16; ++v) {
        const float4 t = *reinterpret_cast<const float4*>(qr + 4 * v);
        const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int c = 0; c < CBD; ++c)
            acc2[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[c][4 * v + i], tv[i], acc2[c], 0, 0, 0);
      }
      // acc2[c][i] = (q W1)[row 16 j + r][column (db0 + c) 16 + 4 kq + i]
      const int64_t R = g * kHsTR + j * 16 + r;
      if (R < rows) {
        const int64_t n = R / M;
        const int m = static_cast<int>(R - n * M);
        const float bt = bm[j * 16 + r];
#pragma unroll
        for (int c = 0; c < CBD; ++c) {
          const int col = (db0 + c) * 16 + 4 * kq;
          const float4 gv = *reinterpret_cast<const float4*>(gy + n * ldg + col);
          float4 o;
          o.x = fmaf(bt, gv.x, acc2[c][0]);
          o.y = fmaf(bt, gv.y, acc2[c][1]);
          o.z = fmaf(bt, gv.z, acc2[c][2]);
          o.w = fmaf(bt, gv.w, acc2[c][3]);
          *reinterpret_cast<float4*>(dz + n * ldd_n + m * ldd_m + col) = o;
        }
      }
    }
  }
}

// adjoint (c), parameter side: workgroup b's dW1 [S, D], db1 [S], dw2 [S] at
// part + b (S D + 2 S). GEMM1 with the operands swapped leaves rows on the accumulator
// registers: acc[cb][i] = (W1 z)[row 16 j + 4 kq + i][column (2 wv + cb) 16 + r], which is the
// A operand of dW1[s][d] += sum_row q[row][s] z[row][d] for k-step i as it stands.
template <int D>
__global__ __launch_bounds__(kHsBlock) void han_dparam_kernel(
    const float* __restrict__ z, int64_t ld_n, int64_t ld_m, int64_t rows, int M,
    const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
    const float* __restrict__ coef, float* __restrict__ part) {
  using T = HsTile<D>;
  constexpr int KS = T::KS;
  constexpr int NB = D / 16;
  __shared__ float xt[kHsTR * T::LDA];
  __shared__ float cm[kHsTR];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int kq = lane >> 4, r = lane & 15;
  float wa[2][KS];
  T::load_w1(wa, w1, wv, kq, r);
  float b1v[2], w2v[2];  // hidden column (2 wv + cb) 16 + r
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
    b1v[cb] = b1[(wv * 2 + cb) * 16 + r];
    w2v[cb] = w2[(wv * 2 + cb) * 16 + r];
  }
  hs4 dw[2][NB];
#pragma unroll
  for (int cb = 0; cb < 2; ++cb)
#pragma unroll
    for (int c = 0; c < NB; ++c) dw[cb][c] = hs4{0.f, 0.f, 0.f, 0.f};
  // db1 and dw2 of this lane's column and rows: a tile's 16 terms in float, the tiles in double
  double dbd[2] = {0.0, 0.0}, d2d[2] = {0.0, 0.0};
  const int64_t tiles = (rows + kHsTR - 1) / kHsTR;
  float4 pre[T::NV];
  T::fetch(pre, z, ld_n, ld_m, rows, M, blockIdx.x);
  for (int64_t g = blockIdx.x; g < tiles; g += gridDim.x) {
    __syncthreads();
    T::stage(xt, pre);
    hs_row_consts(cm, nullptr, coef, nullptr, g, rows, M);
    __syncthreads();
    T::fetch(pre, z, ld_n, ld_m, rows, M, g + gridDim.x);
    float db[2] = {0.f, 0.f}, d2[2] = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < kHsTR / 16; ++j) {
      float xb[KS];
      T::load_x(xb, xt, j, kq, r);
      hs4 acc[2] = {hs4{0.f, 0.f, 0.f, 0.f}, hs4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
          acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xb[s], wa[cb][s], acc[cb], 0, 0, 0);
      hs4 q[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float c = cm[j * 16 + 4 * kq + i];  // 0 past the end: such rows add nothing
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          const float t = han_tanh(acc[cb][i] + b1v[cb]);
          q[cb][i] = c * w2v[cb] * (1.f - t * t);
          db[cb] += q[cb][i];
          d2[cb] = fmaf(c, t, d2[cb]);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int rr = j * 16 + 4 * kq + i;
#pragma unroll
        for (int c = 0; c < NB; ++c) {
          const float zv = T::elem(xt, rr, c * 16 + r);
#pragma unroll
          for (int cb = 0; cb < 2; ++cb)
            dw[cb][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(q[cb][i], zv, dw[cb][c], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      dbd[cb] += static_cast<double>(db[cb]);
      d2d[cb] += static_cast<double>(d2[cb]);
    }
  }
  float* mine = part + static_cast<int64_t>(blockIdx.x) * (kHsS * D + 2 * kHsS);
  // dw[cb][c][i] = dW1[(2 wv + cb) 16 + 4 kq + i][c 16 + r]
#pragma unroll
  for (int cb = 0; cb < 2; ++cb) {
#pragma unroll
    for (int c = 0; c < NB; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        mine[((wv * 2 + cb) * 16 + 4 * kq + i) * D + c * 16 + r] = dw[cb][c][i];
    double a = dbd[cb], b = d2d[cb];  // the four lane quarters hold different rows
    a += hs_shfl_xor_d(a, 16);
    a += hs_shfl_xor_d(a, 32);
    b += hs_shfl_xor_d(b, 16);
    b += hs_shfl_xor_d(b, 32);
    if (kq == 0) {
      mine[kHsS * D + (wv * 2 + cb) * 16 + r] = static_cast<float>(a);
      mine[kHsS * D + kHsS + (wv * 2 + cb) * 16 + r] = static_cast<float>(b);
    }
  }
}

// element e of [dW1 | db1 | dw2], 64 elements per workgroup: wave w adds the partials of
// workgroups w, w + 4, ... in that order (double), the four sums are added in wave order
__global__ __launch_bounds__(kHsBlock) void han_param_reduce_kernel(
    const float* __restrict__ part, int nb, int D, float* __restrict__ dw1,
    float* __restrict__ db1, float* __restrict__ dw2) {
  __shared__ double ws[kHsBlock / kWave][kWave];
  const int per = kHsS * D + 2 * kHsS;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int e = blockIdx.x * kWave + lane;
  double t = 0.0;
  if (e < per) {
#pragma unroll 8
    for (int b = wv; b < nb; b += kHsBlock / kWave)
      t += static_cast<double>(part[static_cast<int64_t>(b) * per + e]);
  }
  ws[wv][lane] = t;
  __syncthreads();
  if (wv != 0 || e >= per) return;
  const float v = static_cast<float>(((ws[0][lane] + ws[1][lane]) + ws[2][lane]) + ws[3][lane]);
  if (e < kHsS * D) {
    if (dw1) dw1[e] = v;
  } else if (e < kHsS * D + kHsS) {
    if (db1) db1[e - kHsS * D] = v;
  } else if (dw2) {
    dw2[e - kHsS * D - kHsS] = v;
  }
}

__global__ __launch_bounds__(kHsBlock) void han_tanh_kernel(const float* __restrict__ x,
                                                            float* __restrict__ y, int64_t n) {
  const int64_t step = static_cast<int64_t>(gridDim.x) * kHsBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kHsBlock + threadIdx.x; i < n; i += step)
    y[i] = han_tanh(x[i]);
}

// workspace: [0, 32 KiB) the 512 x 8 double partials of the scores / dbeta pass, then 8 floats
// of coefficients (64 B), then the parameter kernel's partials
constexpr int64_t kHsPartBytes = static_cast<int64_t>(kHsGrid) * kHsMaxM * 8;
constexpr int64_t kHsCoefBytes = 64;

static unsigned hs_stream_grid(int64_t total) {
  const int64_t nb = (total + kHsBlock - 1) / kHsBlock;
  return static_cast<unsigned>(nb < 1 ? 1 : nb > 4096 ? 4096 : nb);
}

}  // namespace gnn

using namespace gnn;

extern "C" int gnn_han_semantic_supported(int64_t D, int64_t S, int64_t M) {
  const bool d = D == 16 || D == 32 || D == 64 || D == 128;
  return d && S == kHsS && M >= 1 && M <= kHsMaxM;
}

extern "C" int64_t gnn_han_semantic_workspace_bytes(int64_t N, int64_t M, int64_t D, int64_t S) {
  if (N < 0 || M < 0 || D < 0 || S < 0) return GNN_E_ARG;
  if (!gnn_han_semantic_supported(D, S, M)) return GNN_E_UNSUPPORTED;
  if (N > INT64_MAX / 16 / M) return GNN_E_UNSUPPORTED;
  const int64_t pg = hs_grid(N * M, kHsParamGrid);
  return kHsPartBytes + kHsCoefBytes + pg * (S * D + 2 * S) * 4;
}

extern "C" int gnn_han_semantic_fwd_f32(const float* z, int64_t ld_n, int64_t ld_m, int64_t N,
                                        int64_t M, int64_t D, int64_t S, const float* w1,
                                        const float* b1, const float* w2, float* w, float* beta,
                                        float* out, int64_t ldo, void* ws, int64_t ws_bytes,
                                        void* stream) {
  if (N < 0 || M < 0 || D < 0 || S < 0) return GNN_E_ARG;
  if (!gnn_han_semantic_supported(D, S, M)) return GNN_E_UNSUPPORTED;
  if (ld_m < D || ld_n / M < ld_m || ldo < D) return GNN_E_ARG;
  if (N > 0 && (!z || !w1 || !b1 || !w2 || !beta || !out || !ws)) return GNN_E_ARG;
  if (N > INT64_MAX / 16 / ld_n || N > INT64_MAX / 16 / ldo) return GNN_E_UNSUPPORTED;
  if (N > 0 && ws_bytes < gnn_han_semantic_workspace_bytes(N, M, D, S)) return GNN_E_ARG;
  if (ld_n % 4 || ld_m % 4 || ldo % 4 || !aligned_to(z, 16) || !aligned_to(w1, 16) ||
      !aligned_to(b1, 4) || !aligned_to(w2, 4) || !aligned_to(w, 4) || !aligned_to(beta, 4) ||
      !aligned_to(out, 16) || !aligned_to(ws, 8))
    return GNN_E_ALIGN;
  if (N == 0) return GNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t rows = N * M;
  const int m = static_cast<int>(M);
  const int nb = hs_grid(rows, kHsGrid);
  double* part = static_cast<double*>(ws);
#define HS_SCORES(DD)                                                                        \
  case DD:                                                                                   \
    hipLaunchKernelGGL(han_scores_kernel<DD>, dim3(nb), dim3(kHsBlock), 0, s, z, ld_n, ld_m, \
                       rows, m, w1, b1, w2, part);                                           \
    break
  switch (D) {
    HS_SCORES(16);
    HS_SCORES(32);
    HS_SCORES(64);
    HS_SCORES(128);
  }
#undef HS_SCORES
  hipLaunchKernelGGL(han_finish_kernel, dim3(1), dim3(kWave), 0, s, part, nb, m, N, w, beta);
  hipLaunchKernelGGL(han_combine_kernel, dim3(hs_stream_grid(N * (D / 4))), dim3(kHsBlock), 0, s,
                     z, ld_n, ld_m, N, m, static_cast<int>(D / 4), beta, out, ldo);
  return launch_status();
}

extern "C" int gnn_han_semantic_bwd_f32(const float* g, int64_t ldg, const float* z, int64_t ld_n,
                                        int64_t ld_m, int64_t N, int64_t M, int64_t D, int64_t S,
                                        const float* w1, const float* b1, const float* w2,
                                        const float* beta, float* dz, int64_t lddz_n,
                                        int64_t lddz_m, float* dw1, float* db1, float* dw2,
                                        void* ws, int64_t ws_bytes, void* stream) {
  if (N < 0 || M < 0 || D < 0 || S < 0) return GNN_E_ARG;
  if (!gnn_han_semantic_supported(D, S, M)) return GNN_E_UNSUPPORTED;
  if (ld_m < D || ld_n / M < ld_m || ldg < D) return GNN_E_ARG;
  if (dz && (lddz_m < D || lddz_n / M < lddz_m)) return GNN_E_ARG;
  if (N > 0 && (!g || !z || !w1 || !b1 || !w2 || !beta || !ws)) return GNN_E_ARG;
  if (N > INT64_MAX / 16 / ld_n || N > INT64_MAX / 16 / ldg ||
      (dz && N > INT64_MAX / 16 / lddz_n))
    return GNN_E_UNSUPPORTED;
  if (N > 0 && ws_bytes < gnn_han_semantic_workspace_bytes(N, M, D, S)) return GNN_E_ARG;
  if (ld_n % 4 || ld_m % 4 || ldg % 4 || (dz && (lddz_n % 4 || lddz_m % 4)) ||
      !aligned_to(g, 16) || !aligned_to(z, 16) || !aligned_to(w1, 16) || !aligned_to(b1, 4) ||
      !aligned_to(w2, 4) || !aligned_to(beta, 4) || !aligned_to(dz, 16) || !aligned_to(dw1, 4) ||
      !aligned_to(db1, 4) || !aligned_to(dw2, 4) || !aligned_to(ws, 8))
    return GNN_E_ALIGN;
  if (N == 0) return GNN_OK;
  const bool params = dw1 || db1 || dw2;
  if (!dz && !params) return GNN_OK;  // nothing asked for
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t rows = N * M;
  const int m = static_cast<int>(M), d = static_cast<int>(D);
  double* part = static_cast<double*>(ws);
  float* coef = reinterpret_cast<float*>(static_cast<char*>(ws) + kHsPartBytes);
  float* ppart = reinterpret_cast<float*>(static_cast<char*>(ws) + kHsPartBytes + kHsCoefBytes);
  const int fb = hs_flat_grid(N, D);
  hipLaunchKernelGGL(han_dbeta_kernel, dim3(fb), dim3(kHsBlock), 0, s, g, ldg, z, ld_n, ld_m, N,
                     m, d / 4, part);
  hipLaunchKernelGGL(han_coef_kernel, dim3(1), dim3(kWave), 0, s, part, fb, m, N, beta, coef);
  const int nb = hs_grid(rows, kHsGrid), pb = hs_grid(rows, kHsParamGrid);
#define HS_BWD(DD)                                                                             \
  case DD:                                                                                     \
    if (dz)                                                                                    \
      hipLaunchKernelGGL(han_dz_kernel<DD>, dim3(nb), dim3(kHsBlock), 0, s, z, ld_n, ld_m,     \
                         rows, m, w1, b1, w2, coef, beta, g, ldg, dz, lddz_n, lddz_m);         \
    if (params)                                                                                \
      hipLaunchKernelGGL(han_dparam_kernel<DD>, dim3(pb), dim3(kHsBlock), 0, s, z, ld_n, ld_m, \
                         rows, m, w1, b1, w2, coef, ppart);                                    \
    break
  switch (D) {
    HS_BWD(16);
    HS_BWD(32);
    HS_BWD(64);
    HS_BWD(128);
  }
#undef HS_BWD
  if (params) {
    const int per = kHsS * d + 2 * kHsS;
    hipLaunchKernelGGL(han_param_reduce_kernel, dim3((per + kWave - 1) / kWave),
                       dim3(kHsBlock), 0, s, ppart, pb, d, dw1, db1, dw2);
  }
  return launch_status();
}

// y[i] = the kernels' tanh of x[i] (1 - 2 / (1 + exp(2x)) on the hardware exponential and
// reciprocal): what tests/test_han_semantic_gpu.py measures against float64
extern "C" int gnn_han_tanh_f32(const float* x, float* y, int64_t n, void* stream) {
  if (n < 0) return GNN_E_ARG;
  if (n > 0 && (!x || !y)) return GNN_E_ARG;
  if (!aligned_to(x, 4) || !aligned_to(y, 4)) return GNN_E_ALIGN;
  if (n == 0) return GNN_OK;
  hipLaunchKernelGGL(han_tanh_kernel, dim3(hs_stream_grid(n)), dim3(kHsBlock), 0,
                     static_cast<hipStream_t>(stream), x, y, n);
  return launch_status();
}
