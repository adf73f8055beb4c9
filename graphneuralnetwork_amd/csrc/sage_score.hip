// sage_score.hip -- the head of the unsupervised GraphSAGE step on gfx950
// (GraphSAGE/GraphSAGE.py:61 torch.bmm(center.unsqueeze(1), second.permute(0, 2, 1)) and
// GraphSAGE/train_eval.py:113-114 binary_cross_entropy_with_logits over its scores).
//
// c is the centre embeddings [B, H], x the second tower's embeddings [B S, H] (row b S + s).
//
//   gnn_sage_score_f32: z[b, s] = sum_h c[b, h] x[b S + s, h]. One wavefront per b; its
//     64 / (H/4) lane groups of H/4 lanes take the s values round robin, each lane holding
//     floats [4 sub, 4 sub + 4) of c_b (loaded once) and of the rows it meets (16-B loads,
//     kScU rows in flight per group). The group's sum is a fixed xor-shuffle tree.
//   gnn_sage_score_bwd_f32: the same walk. dx[b S + s] = g[b, s] c[b] is one product per
//     element, stored straight in the [B S, H] layout; dc[b] = sum_s g[b, s] x[b S + s] is
//     summed by every group over its own s values in ascending order, then the groups' partial
//     rows are added by xor-shuffles across the groups: the order is a function of (S, H) alone.
//   gnn_bce_logits_f32: mean of (1 - y) z - logsigmoid(z) and its gradient. A fixed grid of
//     blocks (a function of n alone) sums its elements in double in a fixed order and writes
//     one partial per block; a second launch of one wavefront adds the partials in a fixed
//     order. Each element is evaluated in double and rounded once.
// No floating-point atomics anywhere: every result is bit-identical from run to run.
#include "common.hpp"

namespace gnn {

constexpr int kScBlock = 256;
constexpr int kScWaves = kScBlock / kWave;
constexpr int kScU = 4;  // rows in flight per lane group

template <int LPR>
__global__ __launch_bounds__(kScBlock) void sage_score_kernel(
    const float* __restrict__ c, int64_t ldc, const float* __restrict__ x, int64_t ldx, int64_t B,
    int64_t S, float* __restrict__ z, int64_t ldz) {
  constexpr int G = kWave / LPR;  // lane groups per wavefront
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kScWaves + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane % LPR, grp = lane / LPR;
  const f4 cb = vload<4>(c + b * ldc + 4 * sub);
  const float* xb = x + b * S * ldx + 4 * sub;
  float* zb = z + b * ldz;
  for (int64_t s0 = grp; s0 < S; s0 += static_cast<int64_t>(G) * kScU) {
    f4 v[kScU];
#pragma unroll
    for (int u = 0; u < kScU; ++u) {
      const int64_t s = s0 + static_cast<int64_t>(u) * G;
      v[u] = s < S ? vload<4>(xb + s * ldx) : vzero<4>();
    }
    float p[kScU];
#pragma unroll
    for (int u = 0; u < kScU; ++u) {
      p[u] = cb.x * v[u].x + cb.y * v[u].y + cb.z * v[u].z + cb.w * v[u].w;
#pragma unroll
      for (int m = 1; m < LPR; m <<= 1) p[u] += shfl_xor_f(p[u], m);
    }
    if (sub == 0) {
#pragma unroll
      for (int u = 0; u < kScU; ++u) {
        const int64_t s = s0 + static_cast<int64_t>(u) * G;
        if (s < S) zb[s] = p[u];
      }
    }
  }
}

template <int LPR, bool DC, bool DX>
__global__ __launch_bounds__(kScBlock) void sage_score_bwd_kernel(
    const float* __restrict__ g, int64_t ldg, const float* __restrict__ c, int64_t ldc,
    const float* __restrict__ x, int64_t ldx, int64_t B, int64_t S, float* __restrict__ dc,
    int64_t lddc, float* __restrict__ dx, int64_t lddx) {
  constexpr int G = kWave / LPR;
  const int64_t b = static_cast<int64_t>(blockIdx.x) * kScWaves + (threadIdx.x >> 6);
  if (b >= B) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane % LPR, grp = lane / LPR;
  const float* gb = g + b * ldg;
  f4 cb = vzero<4>();
  if (DX) cb = vload<4>(c + b * ldc + 4 * sub);
  f4 acc = vzero<4>();
  for (int64_t s0 = grp; s0 < S; s0 += static_cast<int64_t>(G) * kScU) {
    f4 v[kScU];
    float gs[kScU];
#pragma unroll
    for (int u = 0; u < kScU; ++u) {
      const int64_t s = s0 + static_cast<int64_t>(u) * G;
      v[u] = vzero<4>();
      gs[u] = 0.f;
      if (s < S) {
        gs[u] = gb[s];
        if (DC) v[u] = vload<4>(x + (b * S + s) * ldx + 4 * sub);
      }
    }
#pragma unroll
    for (int u = 0; u < kScU; ++u) {
      const int64_t s = s0 + static_cast<int64_t>(u) * G;
      if (s < S) {  // a row past S adds nothing (its zeros would turn an Inf gradient into NaN)
        if (DC) acc += v[u] * gs[u];
        if (DX) vstore<4>(dx + (b * S + s) * lddx + 4 * sub, cb * gs[u]);
      }
    }
  }
  if (DC) {
#pragma unroll
    for (int m = LPR; m < kWave; m <<= 1) acc += shfl_xor_f(acc, m);
    if (lane < LPR) vstore<4>(dc + b * lddc + 4 * sub, acc);
  }
}

template <int LPR>
static int launch_sage_score(const float* c, int64_t ldc, const float* x, int64_t ldx, int64_t B,
                             int64_t S, float* z, int64_t ldz, hipStream_t s) {
  const int64_t blocks = (B + kScWaves - 1) / kScWaves;
  hipLaunchKernelGGL(sage_score_kernel<LPR>, dim3(static_cast<unsigned>(blocks)), dim3(kScBlock),
                     0, s, c, ldc, x, ldx, B, S, z, ldz);
  return launch_status();
}

template <int LPR>
static int launch_sage_score_bwd(const float* g, int64_t ldg, const float* c, int64_t ldc,
                                 const float* x, int64_t ldx, int64_t B, int64_t S, float* dc,
                                 int64_t lddc, float* dx, int64_t lddx, hipStream_t s) {
  const dim3 grid(static_cast<unsigned>((B + kScWaves - 1) / kScWaves)), block(kScBlock);
  if (dc && dx)
    hipLaunchKernelGGL((sage_score_bwd_kernel<LPR, true, true>), grid, block, 0, s, g, ldg, c, ldc,
                       x, ldx, B, S, dc, lddc, dx, lddx);
  else if (dc)
    hipLaunchKernelGGL((sage_score_bwd_kernel<LPR, true, false>), grid, block, 0, s, g, ldg, c,
                       ldc, x, ldx, B, S, dc, lddc, dx, lddx);
  else
    hipLaunchKernelGGL((sage_score_bwd_kernel<LPR, false, true>), grid, block, 0, s, g, ldg, c,
                       ldc, x, ldx, B, S, dc, lddc, dx, lddx);
  return launch_status();
}

// ---- binary cross entropy with logits ----
constexpr int kBceBlock = 256;
constexpr int kBceMaxBlocks = 1024;
constexpr int kBcePerThread = 4;  // elements per thread before another block is added

static int64_t bce_blocks(int64_t n) {
  int64_t nb = (n + kBceBlock * kBcePerThread - 1) / (kBceBlock * kBcePerThread);
  return nb < 1 ? 1 : nb > kBceMaxBlocks ? kBceMaxBlocks : nb;
}

__device__ __forceinline__ double shfl_xor_d(double v, int m) { return __shfl_xor(v, m, kWave); }

// torch's expression, evaluated in double: (1 - y) z - logsigmoid(z),
// logsigmoid(z) = min(z, 0) - log1p(exp(-|z|)). (z, y) = (+inf, 1), (+inf, 0), (-inf, 1),
// (-inf, 0) give NaN, inf, NaN, NaN as torch does.
__device__ __forceinline__ double bce_term(double z, double y) {
  const double ls = (z < 0.0 ? z : 0.0) - log1p(exp(-fabs(z)));
  return (1.0 - y) * z - ls;
}
__device__ __forceinline__ double sigmoid_d(double z) {
  if (z >= 0.0) return 1.0 / (1.0 + exp(-z));
  const double e = exp(z);  // NaN arrives here and stays NaN
  return e / (1.0 + e);
}

template <bool Y64, bool WIDE>
__global__ __launch_bounds__(kBceBlock) void bce_logits_kernel(
    const float* __restrict__ z, int64_t ldz, const void* __restrict__ yv, int64_t ldy,
    int64_t cols, int64_t n, float* __restrict__ g, int64_t ldg, double* __restrict__ part) {
  __shared__ double wsum[kBceBlock / kWave];
  const float* yf = static_cast<const float*>(yv);
  const int64_t* yi = static_cast<const int64_t*>(yv);
  const double inv_n = 1.0 / static_cast<double>(n);
  const int64_t step = static_cast<int64_t>(gridDim.x) * kBceBlock;
  double acc = 0.0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBceBlock + threadIdx.x; i < n; i += step) {
    int64_t r, col;
    if (WIDE) {
      r = i / cols;
      col = i - r * cols;
    } else {  // n < 2^31: one 32-bit division
      const uint32_t r32 = static_cast<uint32_t>(i) / static_cast<uint32_t>(cols);
      r = r32;
      col = static_cast<uint32_t>(i) - r32 * static_cast<uint32_t>(cols);
    }
    const double zz = static_cast<double>(z[r * ldz + col]);
    const double yy = Y64 ? static_cast<double>(yi[r * ldy + col])
                          : static_cast<double>(yf[r * ldy + col]);
    acc += bce_term(zz, yy);
    if (g) g[r * ldg + col] = static_cast<float>((sigmoid_d(zz) - yy) * inv_n);
  }
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) acc += shfl_xor_d(acc, m);
  if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = wsum[0];
#pragma unroll
    for (int w = 1; w < kBceBlock / kWave; ++w) t += wsum[w];
    part[blockIdx.x] = t;
  }
}

// one wavefront: lane l adds partials l, l + 64, ... in that order, then a fixed xor tree
__global__ __launch_bounds__(kWave) void bce_finish_kernel(const double* __restrict__ part,
                                                           int nb, int64_t n,
                                                           float* __restrict__ loss) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < nb; i += kWave) acc += part[i];
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) acc += shfl_xor_d(acc, m);
  if (threadIdx.x == 0) loss[0] = static_cast<float>(acc / static_cast<double>(n));
}

}  // namespace gnn

using namespace gnn;

extern "C" int gnn_sage_score_supported(int64_t H) {
  // H / 4 lanes per row, a power of two of them per wavefront
  return H >= 4 && H <= 256 && (H & (H - 1)) == 0;
}

// B S ldx and its kin stay inside int64
static bool sc_fits(int64_t B, int64_t S, int64_t ld) {
  if (B == 0 || S == 0) return true;
  if (B > 0x7fffffffLL * kScWaves) return false;
  const int64_t lim = INT64_MAX / 8;
  return S <= lim / B && (B * S) <= lim / ld;
}

extern "C" int gnn_sage_score_f32(const float* c, int64_t ldc, const float* x, int64_t ldx,
                                  int64_t B, int64_t S, int64_t H, float* z, int64_t ldz,
                                  void* stream) {
  if (B < 0 || S < 0 || H < 0) return GNN_E_ARG;
  if (!gnn_sage_score_supported(H)) return GNN_E_UNSUPPORTED;
  if (ldc < H || ldx < H || ldz < S) return GNN_E_ARG;
  if (B > 0 && S > 0 && (!c || !x || !z)) return GNN_E_ARG;
  if (!sc_fits(B, S, ldx) || !sc_fits(B, 1, ldc) || !sc_fits(B, 1, ldz > 0 ? ldz : 1))
    return GNN_E_UNSUPPORTED;
  if (ldc % 4 || ldx % 4 || !aligned_to(c, 16) || !aligned_to(x, 16)) return GNN_E_ALIGN;
  if (B == 0 || S == 0) return GNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (H / 4) {
    case 1: return launch_sage_score<1>(c, ldc, x, ldx, B, S, z, ldz, s);
    case 2: return launch_sage_score<2>(c, ldc, x, ldx, B, S, z, ldz, s);
    case 4: return launch_sage_score<4>(c, ldc, x, ldx, B, S, z, ldz, s);
    case 8: return launch_sage_score<8>(c, ldc, x, ldx, B, S, z, ldz, s);
    case 16: return launch_sage_score<16>(c, ldc, x, ldx, B, S, z, ldz, s);
    case 32: return launch_sage_score<32>(c, ldc, x, ldx, B, S, z, ldz, s);
    default: return launch_sage_score<64>(c, ldc, x, ldx, B, S, z, ldz, s);
  }
}

extern "C" int gnn_sage_score_bwd_f32(const float* g, int64_t ldg, const float* c, int64_t ldc,
                                      const float* x, int64_t ldx, int64_t B, int64_t S,
                                      int64_t H, float* dc, int64_t lddc, float* dx,
                                      int64_t lddx, void* stream) {
  if (B < 0 || S < 0 || H < 0) return GNN_E_ARG;
  if (!gnn_sage_score_supported(H)) return GNN_E_UNSUPPORTED;
  if (ldg < S || (dc && (ldx < H || lddc < H)) || (dx && (ldc < H || lddx < H))) return GNN_E_ARG;
  if (B > 0 && S > 0 && (dc || dx) && (!g || (dc && !x) || (dx && !c))) return GNN_E_ARG;
  if ((dc && (!sc_fits(B, S, ldx) || !sc_fits(B, 1, lddc))) ||
      (dx && (!sc_fits(B, S, lddx) || !sc_fits(B, 1, ldc))) || !sc_fits(B, 1, ldg > 0 ? ldg : 1))
    return GNN_E_UNSUPPORTED;
  if ((dc && (ldx % 4 || lddc % 4 || !aligned_to(x, 16) || !aligned_to(dc, 16))) ||
      (dx && (ldc % 4 || lddx % 4 || !aligned_to(c, 16) || !aligned_to(dx, 16))))
    return GNN_E_ALIGN;
  if (B == 0 || S == 0 || (!dc && !dx)) return GNN_OK;  // S = 0: dc's empty sums are the caller's
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (H / 4) {
    case 1: return launch_sage_score_bwd<1>(g, ldg, c, ldc, x, ldx, B, S, dc, lddc, dx, lddx, s);
    case 2: return launch_sage_score_bwd<2>(g, ldg, c, ldc, x, ldx, B, S, dc, lddc, dx, lddx, s);
    case 4: return launch_sage_score_bwd<4>(g, ldg, c, ldc, x, ldx, B, S, dc, lddc, dx, lddx, s);
    case 8: return launch_sage_score_bwd<8>(g, ldg, c, ldc, x, ldx, B, S, dc, lddc, dx, lddx, s);
    case 16:
      return launch_sage_score_bwd<16>(g, ldg, c, ldc, x, ldx, B, S, dc, lddc, dx, lddx, s);
    case 32:
      return launch_sage_score_bwd<32>(g, ldg, c, ldc, x, ldx, B, S, dc, lddc, dx, lddx, s);
    default:
      return launch_sage_score_bwd<64>(g, ldg, c, ldc, x, ldx, B, S, dc, lddc, dx, lddx, s);
  }
}

extern "C" int64_t gnn_bce_logits_workspace_bytes(int64_t n) {
  if (n < 0) return GNN_E_ARG;
  return (bce_blocks(n) * static_cast<int64_t>(sizeof(double)) + 255) / 256 * 256;
}

extern "C" int gnn_bce_logits_f32(const float* z, int64_t ldz, const void* y, int64_t ldy,
                                  int32_t y_is_i64, int64_t rows, int64_t cols, float* loss,
                                  float* g, int64_t ldg, void* ws, int64_t ws_bytes,
                                  void* stream) {
  if (rows <= 0 || cols <= 0 || !z || !y || !loss || !ws) return GNN_E_ARG;  // no mean of nothing
  if (ldz < cols || ldy < cols || (g && ldg < cols)) return GNN_E_ARG;
  const int64_t lim = INT64_MAX / 16;
  if (rows > lim / cols || rows > lim / ldz || rows > lim / ldy || (g && rows > lim / ldg))
    return GNN_E_UNSUPPORTED;
  const int64_t n = rows * cols;
  if (ws_bytes < gnn_bce_logits_workspace_bytes(n)) return GNN_E_ARG;
  if (!aligned_to(z, 4) || !aligned_to(y, y_is_i64 ? 8 : 4) || !aligned_to(loss, 4) ||
      !aligned_to(g, 4) || !aligned_to(ws, 8))
    return GNN_E_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nb = static_cast<int>(bce_blocks(n));
  double* part = static_cast<double*>(ws);
  const bool wide = n > 0x7fffffffLL;
  const dim3 grid(nb), block(kBceBlock);
  if (y_is_i64) {
    if (wide)
      hipLaunchKernelGGL((bce_logits_kernel<true, true>), grid, block, 0, s, z, ldz, y, ldy, cols,
                         n, g, ldg, part);
    else
      hipLaunchKernelGGL((bce_logits_kernel<true, false>), grid, block, 0, s, z, ldz, y, ldy, cols,
                         n, g, ldg, part);
  } else {
    if (wide)
      hipLaunchKernelGGL((bce_logits_kernel<false, true>), grid, block, 0, s, z, ldz, y, ldy, cols,
                         n, g, ldg, part);
    else
      hipLaunchKernelGGL((bce_logits_kernel<false, false>), grid, block, 0, s, z, ldz, y, ldy,
                         cols, n, g, ldg, part);
  }
  hipLaunchKernelGGL(bce_finish_kernel, dim3(1), dim3(kWave), 0, s, part, nb, n, loss);
  return launch_status();
}
