// gatne.hip -- GATNE's encoder (GATNE_Pytorch/models/GATNE.py GraphEncoder.forward) on gfx950
// without the per-row weight gathers trans_weights[node_types], trans_weights_s1[node_types],
// trans_weights_s2[node_types] ([B, U, E] and [B, U, A] tensors in the reference):
//
//   gnn_typed_gather_sum_f32   u[b, t] = scale * sum_k table[nbr[b, t, k], t]: one lane group per
//                              (b, t), 16-B loads, four neighbour rows in flight, k order.
//   gnn_gatne_order            rows sorted by edge type (stable rocPRIM radix sort over the bits
//                              of T) and the segment offsets; a type outside [0, T) sorts last.
//   gnn_gatne_attend_fwd_f32   tiles of 16 sorted rows of ONE type r: the [16 T, U] tile of u in
//                              LDS, s_t = tanh(u_t W1[r]) . w2[r] on v_mfma_f32_16x16x4_f32 (the
//                              W1 fragment of a column block in registers over all t), softmax
//                              over t, v = sum_t alpha_t u_t, e = c + v M[r], out = e / max(|e|, eps).
//   gnn_gatne_attend_bwd_f32   the same tiles: de from (g, out, inv), dv = de M[r]^T,
//                              dalpha_t = dv . u_t, the tanh recomputed, dz_t = ds_t w2 (1 - h^2),
//                              du_t = alpha_t dv + dz_t W1[r]^T. It leaves v, de and dz in sorted
//                              order; the weight gradients are then TN products over the rows of
//                              a type's segment (gatne_wgrad_kernel): the segment is cut into
//                              kGnSplits row ranges, one partial per (type, range), added in range
//                              order. dw2 is one partial per tile, added in tile order. No
//                              floating-point atomics: bit-identical from run to run.
//
// MFMA operand layout (as han_semantic.hip): lane (kq, r) = (lane >> 4, lane & 15) gives the
// first operand's element (output index r, k-step element kq) and the second operand's (tile row
// r, k-step element kq); acc[i] is (first index 4 kq + i, tile row r).
#include <cstring>  // rocprim's texture_cache_iterator calls host memset
#include <math.h>

#include <rocprim/rocprim.hpp>

#include "common.hpp"
#include "host.hpp"

extern "C" int gnn_gatne_supported(int64_t E, int64_t U, int64_t A, int64_t T);

namespace gnn {

constexpr int kGnBlock = 256;  // 4 waves
constexpr int kGnRows = 16;    // rows per tile
constexpr int kGnMaxT = 8;
constexpr int kGnSplits = 16;  // row ranges per type of the weight-gradient products
constexpr float kGnEps = 1e-12f;        // F.normalize's eps
constexpr float kGnInvClamped = 0.999e12f;  // at or above: inv of a row whose norm was clamped
using gn4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float gn_tanh(float x) {  // han_semantic.hip's han_tanh
  const float e = __expf(2.f * x);
  return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + e);
}

// ---------------------------------------------------------------------------------------
// typed gather-sum: group g = b T + t of G lanes (a power of two <= 64), lane `sub` the float4s
// sub, sub + G, ... of the W / 4
__global__ __launch_bounds__(kGnBlock) void typed_gather_sum_kernel(
    const float* __restrict__ table, int64_t ld_n, int64_t ld_t, int64_t n_table,
    const int64_t* __restrict__ nbr, int64_t BT, int T, int K, int W4, int G, float scale,
    float* __restrict__ u, int64_t ldu, int32_t* __restrict__ err) {
  const int64_t gid = (static_cast<int64_t>(blockIdx.x) * kGnBlock + threadIdx.x) / G;
  const int sub = threadIdx.x % G;
  if (gid >= BT) return;
  const int t = static_cast<int>(gid % T);
  const int64_t* ids = nbr + gid * K;
  const float* base = table + static_cast<int64_t>(t) * ld_t;
  bool bad = false;
  for (int c4 = sub; c4 < W4; c4 += G) {
    f4 acc = vzero<4>();
    for (int k0 = 0; k0 < K; k0 += 4) {
      f4 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = vzero<4>();
        if (k0 + j < K) {
          const int64_t id = ids[k0 + j];
          if (id < 0 || id >= n_table) bad = true;
          else v[j] = vload<4>(base + id * ld_n + 4 * c4);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc += v[j];
    }
    vstore<4>(u + gid * ldu + 4 * c4, acc * scale);
  }
  if (bad && sub == 0) atomicOr(err, 1);
}

// ---------------------------------------------------------------------------------------
// order: keys, sort, segment offsets
__global__ __launch_bounds__(kGnBlock) void gatne_keys_kernel(const int64_t* __restrict__ types,
                                                              int64_t B, int T,
                                                              uint32_t* __restrict__ keys,
                                                              int32_t* __restrict__ status) {
  const int64_t step = static_cast<int64_t>(gridDim.x) * kGnBlock;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kGnBlock + threadIdx.x; i < B; i += step) {
    int64_t t = types[i];
    if (t < 0 || t >= T) {
      atomicOr(status, 1);
      t = T;
    }
    keys[i] = static_cast<uint32_t>(t);
  }
}

// seg[t] = the first position of the sorted keys holding a key >= t, t in [0, T + 1]
__global__ __launch_bounds__(kWave) void gatne_seg_kernel(const uint32_t* __restrict__ keys,
                                                          int64_t B, int T,
                                                          int32_t* __restrict__ seg) {
  const int t = threadIdx.x;
  if (t > T + 1) return;
  int64_t lo = 0, hi = B;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (static_cast<int64_t>(keys[mid]) < t) lo = mid + 1;
    else hi = mid;
  }
  seg[t] = static_cast<int32_t>(lo);
}

static unsigned gn_key_bits(int64_t T) {  // keys in [0, T]
  unsigned b = 1;
  while (b < 32 && (1LL << b) <= T) ++b;
  return b;
}

static size_t gn_sort_temp(int64_t n, unsigned bits) {
  size_t t = 0;
  (void)rocprim::radix_sort_pairs(nullptr, t, static_cast<uint32_t*>(nullptr),
                                  static_cast<uint32_t*>(nullptr),
                                  rocprim::counting_iterator<int32_t>(0),
                                  static_cast<int32_t*>(nullptr), static_cast<size_t>(n), 0, bits);
  return t;
}

struct GnOrderWs {
  uint32_t* k0;
  uint32_t* k1;
  void* temp;
  size_t temp_bytes;
  int64_t bytes;
};
static GnOrderWs gn_order_carve(void* ws, int64_t B, int64_t T) {
  Carve c{static_cast<char*>(ws)};
  GnOrderWs w{};
  w.k0 = c.take<uint32_t>(B);
  w.k1 = c.take<uint32_t>(B);
  w.temp_bytes = gn_sort_temp(B > 0 ? B : 1, gn_key_bits(T));
  w.temp = c.raw(static_cast<int64_t>(w.temp_bytes));
  c.raw(256);
  w.bytes = c.used;
  return w;
}

// ---------------------------------------------------------------------------------------
// the tile of a workgroup: tiles are numbered type by type (type T = the rows of no type),
// ceil(rows / 16) per type. false for a surplus workgroup or offsets that are not a partition.
__device__ __forceinline__ bool gn_tile(const int32_t* __restrict__ seg, int T, int B, int tile,
                                        int& type, int& p0, int& nrows) {
  int first = 0;
  for (int t = 0; t <= T; ++t) {
    const int b = seg[t], e = seg[t + 1];
    if (b < 0 || e < b || e > B) return false;
    const int nt = (e - b + kGnRows - 1) / kGnRows;
    if (tile < first + nt) {
      type = t;
      p0 = b + (tile - first) * kGnRows;
      nrows = e - p0 < kGnRows ? e - p0 : kGnRows;
      return true;
    }
    first += nt;
  }
  return false;
}

struct GnArgs {
  const float* c;  // fwd: the centre rows; bwd: g
  int64_t ldc;
  const float* out;  // bwd
  int64_t ldo_in;
  const float* u;
  const float* alpha_in;  // bwd
  const float* inv_in;    // bwd
  const int32_t* perm;
  const int32_t* seg;
  int B, T, E, A;
  const float* w1;
  const float* w2;
  const float* m;
  // fwd outputs
  float* o;
  int64_t ldo;
  float* alpha;
  float* inv;
  // bwd outputs
  float* dc;
  float* du;
  float* vs;    // [B, U] sorted
  float* ds;    // [B, E] sorted
  float* zs;    // [B T, A] sorted
  float* dw2p;  // [tiles, A]
};

// the u tile: row R = 16 t + i of U floats in the TileLds<U> layout (swizzle by the row in the
// tile), rows past the tile's end zero
template <int U>
struct GnU {
  static constexpr int KS = U / 4;
  static constexpr int LDA = 4 * TileLds<U>::L4;
  static __device__ __forceinline__ int off(int R, int c4) {
    return R * LDA + 4 * (c4 ^ TileLds<U>::swz(R & 15));
  }
  static __device__ __forceinline__ void load_tile(float* __restrict__ ut,
                                                   const float* __restrict__ u,
                                                   const int* __restrict__ rowb, int T) {
    const int n = T * kGnRows * (U / 4);
    for (int e = threadIdx.x; e < n; e += kGnBlock) {
      const int R = e / (U / 4), c4 = e - R * (U / 4);
      const int t = R >> 4, b = rowb[R & 15];
      f4 v = vzero<4>();
      if (b >= 0) v = vload<4>(u + (static_cast<int64_t>(b) * T + t) * U + 4 * c4);
      vstore<4>(ut + off(R, c4), v);
    }
  }
  // row R, this lane quarter's KS values
  static __device__ __forceinline__ void frag(float (&xb)[KS], const float* __restrict__ ut, int R,
                                              int kq) {
#pragma unroll
    for (int v = 0; v < KS / 4; ++v) {
      const f4 t = vload<4>(ut + off(R, kq * (KS / 4) + v));
      xb[4 * v] = t.x;
      xb[4 * v + 1] = t.y;
      xb[4 * v + 2] = t.z;
      xb[4 * v + 3] = t.w;
    }
  }
};

__device__ __forceinline__ void gn_rows(int* __restrict__ rowb, const int32_t* __restrict__ perm,
                                        int p0, int nrows, int B) {
  if (threadIdx.x < kGnRows) {
    int b = -1;
    if (static_cast<int>(threadIdx.x) < nrows) {
      b = perm[p0 + threadIdx.x];
      if (b < 0 || b >= B) b = -1;
    }
    rowb[threadIdx.x] = b;
  }
}

// how the 4 waves share the A / 16 column blocks of u_t W1 and the T neighbour types
struct GnSplit {
  int cb, abase, tstart, wt;
  __device__ GnSplit(int A, int wv) {
    const int nab = A / 16;
    const int wa = nab < 4 ? nab : 4;
    cb = nab / wa;
    abase = (wv % wa) * cb;
    wt = 4 / wa;
    tstart = wv / wa;
  }
};

// LDS floats of the two kernels
static int64_t gn_fwd_lds(int64_t T, int64_t U, int64_t E, int64_t lda) {
  (void)U;
  return (T * 16 * lda + 16 * lda + 16 * (E + 4) + 4 * kGnMaxT * 16 + kGnMaxT * 16 + 64 + 16) * 4;
}
static int64_t gn_bwd_zfloats(int64_t T, int64_t A, int64_t E) {
  const int64_t z = T * 16 * (A + 4), g = 16 * (E + 4);
  return z > g ? z : g;
}
static int64_t gn_bwd_lds(int64_t T, int64_t A, int64_t E, int64_t lda) {
  return (T * 16 * lda + gn_bwd_zfloats(T, A, E) + 16 * lda + 2 * kGnMaxT * 16 + 4 * A + 16 + 16) *
         4;
}

template <int U>
__global__ __launch_bounds__(kGnBlock) void gatne_fwd_kernel(GnArgs a) {
  using X = GnU<U>;
  constexpr int KS = X::KS, LDA = X::LDA;
  extern __shared__ __attribute__((aligned(16))) char gn_smem[];
  const int T = a.T, A = a.A, E = a.E, LE = E + 4;
  float* ut = reinterpret_cast<float*>(gn_smem);  // [16 T][LDA]
  float* vt = ut + T * 16 * LDA;                  // [16][LDA]
  float* et = vt + 16 * LDA;                      // [16][E + 4]
  float* sp = et + 16 * LE;                       // [4][8][16] score pieces of the waves
  float* al = sp + 4 * kGnMaxT * 16;              // [8][16]
  float* dn = al + kGnMaxT * 16;                  // [16] the rows' denominators (64 reserved)
  int* rowb = reinterpret_cast<int*>(dn + 64);    // [16]
  int type, p0, nrows;
  if (!gn_tile(a.seg, T, a.B, blockIdx.x, type, p0, nrows)) return;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int kq = lane >> 4, r = lane & 15;
  gn_rows(rowb, a.perm, p0, nrows, a.B);
  for (int e = threadIdx.x; e < 4 * kGnMaxT * 16; e += kGnBlock) sp[e] = 0.f;
  __syncthreads();
  if (type >= T) {  // rows of no type: NaN
    const float qn = __builtin_nanf("");
    for (int e = threadIdx.x; e < 16 * E; e += kGnBlock) {
      const int b = rowb[e / E];
      if (b >= 0) a.o[static_cast<int64_t>(b) * a.ldo + e % E] = qn;
    }
    for (int e = threadIdx.x; e < 16 * T; e += kGnBlock) {
      const int b = rowb[e / T];
      if (b >= 0) a.alpha[static_cast<int64_t>(b) * T + e % T] = qn;
    }
    if (threadIdx.x < 16 && rowb[threadIdx.x] >= 0) a.inv[rowb[threadIdx.x]] = qn;
    return;
  }
  X::load_tile(ut, a.u, rowb, T);
  __syncthreads();
  // scores: s[t][row] = sum_a w2[a] tanh((u_t W1)[row][a]), the waves' pieces in sp
  {
    const GnSplit sw(A, wv);
    const float* w1 = a.w1 + static_cast<int64_t>(type) * U * A;
    const float* w2 = a.w2 + static_cast<int64_t>(type) * A;
    for (int cb = 0; cb < sw.cb; ++cb) {
      const int col0 = (sw.abase + cb) * 16;
      float wa[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) wa[s] = w1[static_cast<int64_t>(kq * KS + s) * A + col0 + r];
      float w2v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) w2v[i] = w2[col0 + 4 * kq + i];
      for (int t = sw.tstart; t < T; t += sw.wt) {
        float xb[KS];
        X::frag(xb, ut, t * 16 + r, kq);
        gn4 acc = gn4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s)
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[s], xb[s], acc, 0, 0, 0);
        float p = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) p = fmaf(w2v[i], gn_tanh(acc[i]), p);
        p += __shfl_xor(p, 16, kWave);
        p += __shfl_xor(p, 32, kWave);
        if (kq == 0) sp[(wv * kGnMaxT + t) * 16 + r] += p;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 16) {  // torch.softmax over t: the maximum subtracted
    const int i = threadIdx.x, b = rowb[i];
    float s[kGnMaxT], mx = -INFINITY, den = 0.f;
#pragma unroll
    for (int t = 0; t < kGnMaxT; ++t) {
      s[t] = 0.f;
      if (t < T) {
        s[t] = ((sp[(0 * kGnMaxT + t) * 16 + i] + sp[(1 * kGnMaxT + t) * 16 + i]) +
                sp[(2 * kGnMaxT + t) * 16 + i]) + sp[(3 * kGnMaxT + t) * 16 + i];
        mx = fmaxf(mx, s[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < kGnMaxT; ++t)
      if (t < T) {
        s[t] = expf(s[t] - mx);
        den += s[t];
      }
#pragma unroll
    for (int t = 0; t < kGnMaxT; ++t)
      if (t < T) {
        const float av = s[t] / den;
        al[t * 16 + i] = av;
        if (b >= 0) a.alpha[static_cast<int64_t>(b) * T + t] = av;
      }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 16 * (U / 4); e += kGnBlock) {  // v = sum_t alpha_t u_t
    const int i = e / (U / 4), c4 = e - i * (U / 4);
    f4 acc = vload<4>(ut + X::off(i, c4)) * al[i];
    for (int t = 1; t < T; ++t) acc += vload<4>(ut + X::off(t * 16 + i, c4)) * al[t * 16 + i];
    vstore<4>(vt + X::off(i, c4), acc);
  }
  __syncthreads();
  {  // e = c + v M[type]
    const float* mw = a.m + static_cast<int64_t>(type) * U * E;
    float xb[KS];
    X::frag(xb, vt, r, kq);
    const int b = rowb[r];
    for (int eb = wv; eb < E / 16; eb += 4) {
      float ma[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) ma[s] = mw[static_cast<int64_t>(kq * KS + s) * E + eb * 16 + r];
      gn4 acc = gn4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ma[s], xb[s], acc, 0, 0, 0);
      f4 cv = vzero<4>();
      if (b >= 0) cv = vload<4>(a.c + static_cast<int64_t>(b) * a.ldc + eb * 16 + 4 * kq);
      vstore<4>(et + r * LE + eb * 16 + 4 * kq, f4{cv.x + acc[0], cv.y + acc[1], cv.z + acc[2],
                                                   cv.w + acc[3]});
    }
  }
  __syncthreads();
  {  // out = e / max(|e|, eps): 16 threads per row, float4 chunks j, j + 16, ...
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15, b = rowb[i];
    float ss = 0.f;
    for (int c4 = j; c4 < E / 4; c4 += 16) {
      const f4 v = vload<4>(et + i * LE + 4 * c4);
      ss = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, ss))));
    }
#pragma unroll
    for (int x = 1; x < 16; x <<= 1) ss += __shfl_xor(ss, x, kWave);
    const float den = fmaxf(sqrtf(ss), kGnEps);
    if (b >= 0) {
      for (int c4 = j; c4 < E / 4; c4 += 16) {
        const f4 v = vload<4>(et + i * LE + 4 * c4);
        vstore<4>(a.o + static_cast<int64_t>(b) * a.ldo + 4 * c4,
                  f4{v.x / den, v.y / den, v.z / den, v.w / den});
      }
      if (j == 0) a.inv[b] = 1.f / den;
    }
  }
}

template <int U>
__global__ __launch_bounds__(kGnBlock) void gatne_bwd_kernel(GnArgs a) {
  using X = GnU<U>;
  constexpr int KS = X::KS, LDA = X::LDA;
  extern __shared__ __attribute__((aligned(16))) char gn_smem[];
  const int T = a.T, A = a.A, E = a.E, LE = E + 4, LZ = A + 4;
  float* ut = reinterpret_cast<float*>(gn_smem);  // [16 T][LDA]
  float* zt = ut + T * 16 * LDA;                  // de [16][E + 4], then dz [16 T][A + 4]
  float* dvt = zt + (T * 16 * LZ > 16 * LE ? T * 16 * LZ : 16 * LE);  // [16][LDA]
  float* al = dvt + 16 * LDA;                     // [8][16]
  float* dsl = al + kGnMaxT * 16;                 // [8][16] dalpha, then ds
  float* w2p = dsl + kGnMaxT * 16;                // [4][A] dw2 pieces of the waves
  float* invr = w2p + 4 * A;                      // [16]
  int* rowb = reinterpret_cast<int*>(invr + 16);  // [16]
  int type, p0, nrows;
  if (!gn_tile(a.seg, T, a.B, blockIdx.x, type, p0, nrows)) return;
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int kq = lane >> 4, r = lane & 15;
  gn_rows(rowb, a.perm, p0, nrows, a.B);
  for (int e = threadIdx.x; e < 4 * A; e += kGnBlock) w2p[e] = 0.f;
  __syncthreads();
  if (type >= T) {  // rows of no type: zero gradients
    for (int e = threadIdx.x; e < 16 * E; e += kGnBlock) {
      const int b = rowb[e / E];
      if (b >= 0) a.dc[static_cast<int64_t>(b) * E + e % E] = 0.f;
    }
    if (a.du)
      for (int e = threadIdx.x; e < 16 * T * U; e += kGnBlock) {
        const int b = rowb[e / (T * U)];
        if (b >= 0) a.du[static_cast<int64_t>(b) * T * U + e % (T * U)] = 0.f;
      }
    return;
  }
  X::load_tile(ut, a.u, rowb, T);
  for (int e = threadIdx.x; e < 16 * T; e += kGnBlock) {
    const int t = e >> 4, b = rowb[e & 15];
    al[e] = b >= 0 ? a.alpha_in[static_cast<int64_t>(b) * T + t] : 0.f;
  }
  if (threadIdx.x < 16) invr[threadIdx.x] = rowb[threadIdx.x] >= 0 ? a.inv_in[rowb[threadIdx.x]] : 0.f;
  __syncthreads();
  {  // de = inv (g - out (out . g)); a clamped row: g / eps. 16 threads per row
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15, b = rowb[i];
    f4 gv[4], ov[4];
    float dot = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      gv[q] = vzero<4>();
      ov[q] = vzero<4>();
      const int c4 = j + 16 * q;
      if (b >= 0 && c4 < E / 4) {
        gv[q] = vload<4>(a.c + static_cast<int64_t>(b) * a.ldc + 4 * c4);
        ov[q] = vload<4>(a.out + static_cast<int64_t>(b) * a.ldo_in + 4 * c4);
      }
      dot = fmaf(gv[q].x, ov[q].x, fmaf(gv[q].y, ov[q].y, fmaf(gv[q].z, ov[q].z,
                                                               fmaf(gv[q].w, ov[q].w, dot))));
    }
#pragma unroll
    for (int x = 1; x < 16; x <<= 1) dot += __shfl_xor(dot, x, kWave);
    const float iv = invr[i];
    if (iv >= kGnInvClamped) dot = 0.f;  // F.normalize: the clamped denominator is a constant
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c4 = j + 16 * q;
      if (c4 < E / 4) {
        const f4 de = (gv[q] - ov[q] * dot) * iv;
        vstore<4>(zt + i * LE + 4 * c4, de);
        if (b >= 0) {
          vstore<4>(a.dc + static_cast<int64_t>(b) * E + 4 * c4, de);
          vstore<4>(a.ds + static_cast<int64_t>(p0 + i) * E + 4 * c4, de);
        }
      }
    }
  }
  __syncthreads();
  {  // dv = de M[type]^T: first operand M[16 ub + r][e], second de[r][e], e = kq E / 4 + s
    const float* mw = a.m + static_cast<int64_t>(type) * U * E;
    const int kse = E / 4;
    for (int ub = wv; ub < U / 16; ub += 4) {
      const float* mr = mw + static_cast<int64_t>(ub * 16 + r) * E + kq * kse;
      const float* dr = zt + r * LE + kq * kse;
      gn4 acc = gn4{0.f, 0.f, 0.f, 0.f};

      for (int s4 = 0; s4 < kse / 4; ++s4) {
        const f4 mv = vload<4>(mr + 4 * s4), dv = vload<4>(dr + 4 * s4);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(mv.x, dv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(mv.y, dv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(mv.z, dv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(mv.w, dv.w, acc, 0, 0, 0);
      }
      vstore<4>(dvt + X::off(r, ub * 4 + kq), f4{acc[0], acc[1], acc[2], acc[3]});
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 16 * (U / 4); e += kGnBlock) {  // v, for dM
    const int i = e / (U / 4), c4 = e - i * (U / 4);
    f4 acc = vload<4>(ut + X::off(i, c4)) * al[i];
    for (int t = 1; t < T; ++t) acc += vload<4>(ut + X::off(t * 16 + i, c4)) * al[t * 16 + i];
    if (i < nrows) vstore<4>(a.vs + static_cast<int64_t>(p0 + i) * U + 4 * c4, acc);
  }
  if (static_cast<int>(threadIdx.x) < 16 * T) {  // dalpha[t][i] = dv[i] . u_t[i]
    const int i = threadIdx.x & 15, t = threadIdx.x >> 4;
    float d = 0.f;
    for (int c4 = 0; c4 < U / 4; ++c4) {
      const f4 x = vload<4>(ut + X::off(t * 16 + i, c4)), y = vload<4>(dvt + X::off(i, c4));
      d = fmaf(x.x, y.x, fmaf(x.y, y.y, fmaf(x.z, y.z, fmaf(x.w, y.w, d))));
    }
    dsl[t * 16 + i] = d;
  }
  __syncthreads();
  if (threadIdx.x < 16) {  // ds_t = alpha_t (dalpha_t - sum_k alpha_k dalpha_k)
    const int i = threadIdx.x;
    float da[kGnMaxT], sum = 0.f;
#pragma unroll
    for (int t = 0; t < kGnMaxT; ++t) {
      da[t] = t < T ? dsl[t * 16 + i] : 0.f;
      if (t < T) sum = fmaf(al[t * 16 + i], da[t], sum);
    }
#pragma unroll
    for (int t = 0; t < kGnMaxT; ++t)
      if (t < T) dsl[t * 16 + i] = al[t * 16 + i] * (da[t] - sum);
  }
  __syncthreads();
  {  // h = tanh(u_t W1) again; dz = ds w2 (1 - h^2) into LDS (over de) and the sorted copy
    const GnSplit sw(A, wv);
    const float* w1 = a.w1 + static_cast<int64_t>(type) * U * A;
    const float* w2 = a.w2 + static_cast<int64_t>(type) * A;
    for (int cb = 0; cb < sw.cb; ++cb) {
      const int col0 = (sw.abase + cb) * 16;
      float wa[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) wa[s] = w1[static_cast<int64_t>(kq * KS + s) * A + col0 + r];
      float w2v[4], dq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) w2v[i] = w2[col0 + 4 * kq + i];
      for (int t = sw.tstart; t < T; t += sw.wt) {
        float xb[KS];
        X::frag(xb, ut, t * 16 + r, kq);
        gn4 acc = gn4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s)
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[s], xb[s], acc, 0, 0, 0);
        const float dsr = dsl[t * 16 + r];
        f4 dz;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float h = gn_tanh(acc[i]);
          dz[i] = dsr * w2v[i] * (1.f - h * h);
          float q = dsr * h;  // dw2: summed over the tile's rows (16 lanes), then over t
#pragma unroll
          for (int x = 1; x < 16; x <<= 1) q += __shfl_xor(q, x, kWave);
          dq[i] += q;
        }
        vstore<4>(zt + (t * 16 + r) * LZ + col0 + 4 * kq, dz);
        if (r < nrows)
          vstore<4>(a.zs + (static_cast<int64_t>(p0 + r) * T + t) * A + col0 + 4 * kq, dz);
      }
      if (r == 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) w2p[wv * A + col0 + 4 * kq + i] = dq[i];
    }
  }
  __syncthreads();
  if (a.dw2p && static_cast<int>(threadIdx.x) < A) {
    const int c = threadIdx.x;
    a.dw2p[static_cast<int64_t>(blockIdx.x) * A + c] =
        ((w2p[c] + w2p[A + c]) + w2p[2 * A + c]) + w2p[3 * A + c];
  }
  if (a.du) {  // du_t = alpha_t dv + dz_t W1^T: first operand W1[16 ub + r][a], second dz_t[r][a]
    const float* w1 = a.w1 + static_cast<int64_t>(type) * U * A;
    const int ksa = A / 4, b = rowb[r];
    for (int ub = wv; ub < U / 16; ub += 4) {
      const float* wr = w1 + static_cast<int64_t>(ub * 16 + r) * A + kq * ksa;
      const f4 dvv = vload<4>(dvt + X::off(r, ub * 4 + kq));
      for (int t = 0; t < T; ++t) {
        const float* zr = zt + (t * 16 + r) * LZ + kq * ksa;
        gn4 acc = gn4{0.f, 0.f, 0.f, 0.f};

        for (int s4 = 0; s4 < ksa / 4; ++s4) {
          const f4 wv4 = vload<4>(wr + 4 * s4), zv = vload<4>(zr + 4 * s4);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.x, zv.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.y, zv.y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.z, zv.z, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv4.w, zv.w, acc, 0, 0, 0);
        }
        if (b >= 0) {
          const float at = al[t * 16 + r];
          vstore<4>(a.du + (static_cast<int64_t>(b) * T + t) * U + ub * 16 + 4 * kq,
                    f4{fmaf(at, dvv.x, acc[0]), fmaf(at, dvv.y, acc[1]), fmaf(at, dvv.z, acc[2]),
                       fmaf(at, dvv.w, acc[3])});
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// weight gradients: part[(type G + j)][mdim][ndim] = sum over the rows q of range j of the type's
// segment of X[q, :]^T Y[q, :]. rt rows per sorted position (1: dM, T: dW1); X row q is
// x[(perm[q / rt] rt + q % rt) ldx ..] (batch order) or x[q ldx ..] (perm null); Y is sorted.
// A wave owns one 16-row block of the output and up to four 16-column blocks.
struct GnWgArgs {
  const float* x;
  int64_t ldx;
  const int32_t* perm;
  const float* y;
  int64_t ldy;
  const int32_t* seg;
  int B, T, rt, mdim, ndim;
  float* part;
};

__global__ __launch_bounds__(kGnBlock) void gatne_wgrad_kernel(GnWgArgs a) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int kq = lane >> 4, r = lane & 15;
  const int nbw = a.ndim / 16 < 4 ? a.ndim / 16 : 4;
  const int groups = a.ndim / (16 * nbw);
  const int task = blockIdx.x * 4 + wv;
  if (task >= (a.mdim / 16) * groups) return;
  const int mb = task / groups, ng = task - mb * groups;
  const int type = blockIdx.z, j = blockIdx.y;
  int sb = a.seg[type], se = a.seg[type + 1];
  if (sb < 0 || se < sb || se > a.B) sb = se = 0;
  const int64_t lo = static_cast<int64_t>(sb) * a.rt, hi = static_cast<int64_t>(se) * a.rt;
  const int64_t chunk = (((hi - lo + kGnSplits - 1) / kGnSplits) + 3) & ~static_cast<int64_t>(3);
  const int64_t qb = lo + j * chunk;
  const int64_t qe = qb + chunk < hi ? qb + chunk : hi;
  gn4 acc[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) acc[nb] = gn4{0.f, 0.f, 0.f, 0.f};
  for (int64_t q0 = qb; q0 < qe; q0 += 4) {
    const int64_t q = q0 + kq;
    float av = 0.f, bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (q < qe) {
      int64_t xr = q;
      bool ok = true;
      if (a.perm) {
        const int64_t pos = q / a.rt;
        const int b = a.perm[pos];
        ok = b >= 0 && b < a.B;
        xr = static_cast<int64_t>(b) * a.rt + (q - pos * a.rt);
      }
      if (ok) {
        av = a.x[xr * a.ldx + mb * 16 + r];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
          if (nb < nbw) bv[nb] = a.y[q * a.ldy + (ng * nbw + nb) * 16 + r];
      }
    }
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
      if (nb < nbw) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[nb], acc[nb], 0, 0, 0);
  }
  float* mine = a.part + (static_cast<int64_t>(type) * kGnSplits + j) * a.mdim * a.ndim;
#pragma unroll
  for (int nb = 0; nb < 4; ++nb)
    if (nb < nbw)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        mine[static_cast<int64_t>(mb * 16 + 4 * kq + i) * a.ndim + (ng * nbw + nb) * 16 + r] =
            acc[nb][i];
}

// out[type][e] = the type's kGnSplits partials added in range order
__global__ __launch_bounds__(kGnBlock) void gatne_wreduce_kernel(const float* __restrict__ part,
                                                                 int64_t mn, int64_t total,
                                                                 float* __restrict__ out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kGnBlock + threadIdx.x;
  if (i >= total) return;
  const int64_t type = i / mn, e = i - type * mn;
  const float* p = part + type * kGnSplits * mn + e;
  float v[kGnSplits];
#pragma unroll
  for (int j = 0; j < kGnSplits; ++j) v[j] = p[j * mn];
  float s = v[0];
#pragma unroll
  for (int j = 1; j < kGnSplits; ++j) s += v[j];
  out[i] = s;
}

// dw2[type][c] = the partials of the type's tiles added in tile order
__global__ __launch_bounds__(kGnBlock) void gatne_dw2_kernel(const float* __restrict__ dw2p,
                                                             const int32_t* __restrict__ seg, int T,
                                                             int B, int A, float* __restrict__ dw2) {
  const int type = blockIdx.x, c = threadIdx.x;
  if (c >= A) return;
  int first = 0, nt = 0;
  for (int t = 0; t <= type; ++t) {
    const int b = seg[t], e = seg[t + 1];
    if (b < 0 || e < b || e > B) {
      nt = 0;
      break;
    }
    first += nt;
    nt = (e - b + kGnRows - 1) / kGnRows;
  }
  float s = 0.f;
  for (int k = 0; k < nt; ++k) s += dw2p[static_cast<int64_t>(first + k) * A + c];
  dw2[type * A + c] = s;
}

static int64_t gn_tiles(int64_t B, int64_t T) { return (B + kGnRows - 1) / kGnRows + T + 1; }

// the workspace of the backward: v | de | dz (sorted) | dw2 partials | weight-gradient partials
struct GnBwdWs {
  float* vs;
  float* ds;
  float* zs;
  float* dw2p;
  float* part;
  int64_t bytes;
};
static GnBwdWs gn_bwd_carve(void* ws, int64_t B, int64_t T, int64_t E, int64_t U, int64_t A) {
  Carve c{static_cast<char*>(ws)};
  GnBwdWs w{};
  w.vs = c.take<float>(B * U);
  w.ds = c.take<float>(B * E);
  w.zs = c.take<float>(B * T * A);
  w.dw2p = c.take<float>(gn_tiles(B, T) * A);
  w.part = c.take<float>(T * kGnSplits * U * (E > A ? E : A));
  w.bytes = c.used;
  return w;
}

static int64_t gn_lda(int64_t U) {
  return U == 16 ? 4 * TileLds<16>::L4 : U == 32 ? 4 * TileLds<32>::L4
       : U == 64 ? 4 * TileLds<64>::L4 : 4 * TileLds<128>::L4;
}

template <class K>
static int gn_launch(K kernel, int64_t tiles, int64_t lds, const GnArgs& a, hipStream_t s) {
  if (lds > 65536)
    GNN_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(tiles)), dim3(kGnBlock),
                     static_cast<size_t>(lds), s, a);
  return launch_status();
}

}  // namespace gnn

using namespace gnn;

extern "C" int gnn_typed_gather_sum_f32(const float* table, int64_t ld_n, int64_t ld_t,
                                        int64_t n_table, const int64_t* nbr, int64_t B, int64_t T,
                                        int64_t K, int64_t W, float scale, float* u, int64_t ldu,
                                        int32_t* err_flag, void* stream) {
  if (B < 0 || T < 0 || K < 0 || W < 0 || n_table < 0 || ld_t < 0 || !err_flag) return GNN_E_ARG;
  if (W % 4 || T > 0x7fffffffLL || K > 0x7fffffffLL || W > 0x7fffffffLL) return GNN_E_UNSUPPORTED;
  if (B == 0 || T == 0 || W == 0) return GNN_OK;
  if (!u || ldu < W || (K > 0 && (!table || !nbr))) return GNN_E_ARG;
  if (ld_n < (T - 1) * ld_t + W) return GNN_E_ARG;
  if (B > INT64_MAX / 64 / T || B * T > INT64_MAX / 16 / (ldu > K ? ldu : K) ||
      (n_table > 0 && n_table > INT64_MAX / 16 / ld_n))
    return GNN_E_UNSUPPORTED;
  if (ld_n % 4 || ld_t % 4 || ldu % 4 || !aligned_to(table, 16) || !aligned_to(u, 16) ||
      !aligned_to(nbr, 8))
    return GNN_E_ALIGN;
  const int G = next_pow2_le64(W / 4);
  const int64_t blocks = (B * T * G + kGnBlock - 1) / kGnBlock;
  if (blocks > 0x7fffffffLL) return GNN_E_UNSUPPORTED;
  hipLaunchKernelGGL(typed_gather_sum_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kGnBlock),
                     0, static_cast<hipStream_t>(stream), table, ld_n, ld_t, n_table, nbr, B * T,
                     static_cast<int>(T), static_cast<int>(K), static_cast<int>(W / 4), G, scale, u,
                     ldu, err_flag);
  return launch_status();
}

extern "C" int64_t gnn_gatne_order_workspace_bytes(int64_t B, int64_t T) {
  if (B < 0 || T < 1) return GNN_E_ARG;
  if (T > kGnMaxT || B > 0x7fffffffLL / (16 * T)) return GNN_E_UNSUPPORTED;
  return gn_order_carve(nullptr, B, T).bytes;
}

extern "C" int gnn_gatne_order(const int64_t* types, int64_t B, int64_t T, int32_t* perm,
                               int32_t* seg, int32_t* status, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  if (B < 0 || T < 1 || !seg || !status || !workspace) return GNN_E_ARG;
  if (T > kGnMaxT || B > 0x7fffffffLL / (16 * T)) return GNN_E_UNSUPPORTED;
  if (B > 0 && (!types || !perm)) return GNN_E_ARG;
  const GnOrderWs w = gn_order_carve(workspace, B, T);
  if (workspace_bytes < w.bytes) return GNN_E_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (B > 0) {
    size_t tb = w.temp_bytes;
    hipLaunchKernelGGL(gatne_keys_kernel, dim3(blocks_capped(B)), dim3(kGnBlock), 0, s, types, B,
                       static_cast<int>(T), w.k0, status);
    GNN_TRY(rocprim::radix_sort_pairs(w.temp, tb, w.k0, w.k1,
                                      rocprim::counting_iterator<int32_t>(0), perm,
                                      static_cast<size_t>(B), 0, gn_key_bits(T), s));
  }
  hipLaunchKernelGGL(gatne_seg_kernel, dim3(1), dim3(kWave), 0, s, w.k1, B, static_cast<int>(T),
                     seg);
  return launch_status();
}

extern "C" int gnn_gatne_supported(int64_t E, int64_t U, int64_t A, int64_t T) {
  const auto w = [](int64_t v) { return v == 16 || v == 32 || v == 64 || v == 128; };
  return w(U) && w(A) && (w(E) || E == 256) && T >= 1 && T <= kGnMaxT;
}

extern "C" int64_t gnn_gatne_attend_workspace_bytes(int64_t B, int64_t T, int64_t E, int64_t U,
                                                    int64_t A) {
  if (B < 0 || T < 0 || E < 0 || U < 0 || A < 0) return GNN_E_ARG;
  if (!gnn_gatne_supported(E, U, A, T) || B > 0x7fffffffLL / (16 * T)) return GNN_E_UNSUPPORTED;
  return gn_bwd_carve(nullptr, B, T, E, U, A).bytes;
}

static void gn_common(GnArgs& a, const float* u, const int32_t* perm, const int32_t* seg, int64_t B,
                      int64_t T, int64_t E, int64_t A, const float* w1, const float* w2,
                      const float* m) {
  a.u = u;
  a.perm = perm;
  a.seg = seg;
  a.B = static_cast<int>(B);
  a.T = static_cast<int>(T);
  a.E = static_cast<int>(E);
  a.A = static_cast<int>(A);
  a.w1 = w1;
  a.w2 = w2;
  a.m = m;
}

extern "C" int gnn_gatne_attend_fwd_f32(const float* c, int64_t ldc, const float* u,
                                        const int32_t* perm, const int32_t* seg, int64_t B,
                                        int64_t T, int64_t E, int64_t U, int64_t A, const float* w1,
                                        const float* w2, const float* m, float* out, int64_t ldo,
                                        float* alpha, float* inv, void* stream) {
  if (B < 0 || T < 0 || E < 0 || U < 0 || A < 0) return GNN_E_ARG;
  if (!gnn_gatne_supported(E, U, A, T) || B > 0x7fffffffLL / (16 * T)) return GNN_E_UNSUPPORTED;
  if (B == 0) return GNN_OK;
  if (!c || !u || !perm || !seg || !w1 || !w2 || !m || !out || !alpha || !inv || ldc < E ||
      ldo < E)
    return GNN_E_ARG;
  if (ldc % 4 || ldo % 4 || !aligned_to(c, 16) || !aligned_to(u, 16) || !aligned_to(w1, 16) ||
      !aligned_to(w2, 4) || !aligned_to(m, 16) || !aligned_to(out, 16) || !aligned_to(alpha, 4) ||
      !aligned_to(inv, 4) || !aligned_to(perm, 4) || !aligned_to(seg, 4))
    return GNN_E_ALIGN;
  GnArgs a{};
  gn_common(a, u, perm, seg, B, T, E, A, w1, w2, m);
  a.c = c;
  a.ldc = ldc;
  a.o = out;
  a.ldo = ldo;
  a.alpha = alpha;
  a.inv = inv;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t tiles = gn_tiles(B, T), lds = gn_fwd_lds(T, U, E, gn_lda(U));
  switch (U) {
    case 16: return gn_launch(gatne_fwd_kernel<16>, tiles, lds, a, s);
    case 32: return gn_launch(gatne_fwd_kernel<32>, tiles, lds, a, s);
    case 64: return gn_launch(gatne_fwd_kernel<64>, tiles, lds, a, s);
    default: return gn_launch(gatne_fwd_kernel<128>, tiles, lds, a, s);
  }
}

extern "C" int gnn_gatne_attend_bwd_f32(const float* g, int64_t ldg, const float* out, int64_t ldo,
                                        const float* u, const float* alpha, const float* inv,
                                        const int32_t* perm, const int32_t* seg, int64_t B,
                                        int64_t T, int64_t E, int64_t U, int64_t A, const float* w1,
                                        const float* w2, const float* m, float* dc, float* du,
                                        float* dw1, float* dw2, float* dm, void* ws,
                                        int64_t ws_bytes, void* stream) {
  if (B < 0 || T < 0 || E < 0 || U < 0 || A < 0) return GNN_E_ARG;
  if (!gnn_gatne_supported(E, U, A, T) || B > 0x7fffffffLL / (16 * T)) return GNN_E_UNSUPPORTED;
  if (dw1 && (!dw2 || !dm)) return GNN_E_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (B == 0) {
    if (dw1) {
      GNN_TRY(hipMemsetAsync(dw1, 0, T * U * A * sizeof(float), s));
      GNN_TRY(hipMemsetAsync(dw2, 0, T * A * sizeof(float), s));
      GNN_TRY(hipMemsetAsync(dm, 0, T * U * E * sizeof(float), s));
    }
    return GNN_OK;
  }
  if (!g || !out || !u || !alpha || !inv || !perm || !seg || !w1 || !w2 || !m || !dc || !ws ||
      ldg < E || ldo < E)
    return GNN_E_ARG;
  const GnBwdWs w = gn_bwd_carve(ws, B, T, E, U, A);
  if (ws_bytes < w.bytes) return GNN_E_ARG;
  if (ldg % 4 || ldo % 4 || !aligned_to(g, 16) || !aligned_to(out, 16) || !aligned_to(u, 16) ||
      !aligned_to(w1, 16) || !aligned_to(w2, 4) || !aligned_to(m, 16) || !aligned_to(dc, 16) ||
      !aligned_to(du, 16) || !aligned_to(dw1, 4) || !aligned_to(dw2, 4) || !aligned_to(dm, 4) ||
      !aligned_to(alpha, 4) || !aligned_to(inv, 4) || !aligned_to(perm, 4) ||
      !aligned_to(seg, 4) || !aligned_to(ws, 16))
    return GNN_E_ALIGN;
  GnArgs a{};
  gn_common(a, u, perm, seg, B, T, E, A, w1, w2, m);
  a.c = g;
  a.ldc = ldg;
  a.out = out;
  a.ldo_in = ldo;
  a.alpha_in = alpha;
  a.inv_in = inv;
  a.dc = dc;
  a.du = du;
  a.vs = w.vs;
  a.ds = w.ds;
  a.zs = w.zs;
  a.dw2p = dw1 ? w.dw2p : nullptr;
  const int64_t tiles = gn_tiles(B, T), lds = gn_bwd_lds(T, A, E, gn_lda(U));
  int rc;
  switch (U) {
    case 16: rc = gn_launch(gatne_bwd_kernel<16>, tiles, lds, a, s); break;
    case 32: rc = gn_launch(gatne_bwd_kernel<32>, tiles, lds, a, s); break;
    case 64: rc = gn_launch(gatne_bwd_kernel<64>, tiles, lds, a, s); break;
    default: rc = gn_launch(gatne_bwd_kernel<128>, tiles, lds, a, s); break;
  }
  if (rc != GNN_OK || !dw1) return rc;
  const int iB = static_cast<int>(B), iT = static_cast<int>(T);
  const auto product = [&](const GnWgArgs& p, float* dst) {
    const int nbw = p.ndim / 16 < 4 ? p.ndim / 16 : 4;
    const int tasks = (p.mdim / 16) * (p.ndim / (16 * nbw));
    hipLaunchKernelGGL(gatne_wgrad_kernel, dim3((tasks + 3) / 4, kGnSplits, iT), dim3(kGnBlock), 0,
                       s, p);
    const int64_t mn = static_cast<int64_t>(p.mdim) * p.ndim, total = mn * iT;
    hipLaunchKernelGGL(gatne_wreduce_kernel, dim3(blocks(total, kGnBlock)), dim3(kGnBlock), 0, s,
                       p.part, mn, total, dst);
  };
  // dM[r] = sum_p v[p]^T de[p]; dW1[r] = sum_(p, t) u[perm[p], t]^T dz[p, t]
  product(GnWgArgs{w.vs, U, nullptr, w.ds, E, seg, iB, iT, 1, static_cast<int>(U),
                   static_cast<int>(E), w.part}, dm);
  product(GnWgArgs{u, U, perm, w.zs, A, seg, iB, iT, iT, static_cast<int>(U), static_cast<int>(A),
                   w.part}, dw1);
  hipLaunchKernelGGL(gatne_dw2_kernel, dim3(iT), dim3(kGnBlock), 0, s, w.dw2p, seg, iT, iB,
                     static_cast<int>(A), dw2);
  return launch_status();
}
