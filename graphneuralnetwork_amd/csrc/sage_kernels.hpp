// sage_kernels.hpp -- the GraphSAGE neighbour aggregation of sage.hip / sage_bf16.hip, generic
// over the element type of the gathered table (or pre-gathered neighbour tensor).
//
// T is the element type of src: float, or bf16_t (2-byte storage, the high half of an fp32, so
// the widening is exact and order-preserving: rows.hpp). The accumulators, the argmax order,
// the slot combine and every output -- fp32 values, int64 indices, the fp32 centre rows of the
// concat form -- are the same for every T: after the load all arithmetic is the fp32 kernel's.
// The fp32 instantiations live in sage.hip, the bf16 ones in sage_bf16.hip (see there for the
// lane layout of a bf16 row).
//
// One wavefront per output row m: EPI = 64/LPR neighbour slots x LPR feature
// lanes x VW-wide loads, U slot loads in flight; the slot partials are combined
// with xor-shuffles. For argmax the combine uses the total order
// (NaN first, larger value, smaller index), so the result is exactly torch's
// regardless of the reduction tree.
#pragma once

#include <type_traits>

#include "rows.hpp"

namespace gnn {

constexpr int kSageBlock = 256;
#ifndef GNN_SAGE_U
// neighbour-slot loads in flight per lane. A/B (tools/lib_ab.py --op sage, 10M-row table,
// k = 10, profiles/r01h_sage_u_ab.log): 2: 37.1 us, 4: 35.5, 8: 33.7, 16: 45.8
#define GNN_SAGE_U 8
#endif
#ifndef GNN_SAGE_BF16_U
// the same for a bf16 table (16 lanes per F = 128 row, EPI = 4 slots, so 4 already covers
// k = 10 in one trip). A/B (tools/lib_ab.py --op sage --dtype bf16 --workload ns, 10M-row
// table, k = 10): 4: 28.5 us, 8: 33.4, 16: 49.9
#define GNN_SAGE_BF16_U 4
#endif
constexpr int kSageWaves = kSageBlock / kWave;

// elements per lane on the vector path (one 16-B load) and slot loads in flight at NCH = 1
template <typename T> struct SageElem;
template <> struct SageElem<float> { static constexpr int kVec = 4, kU = GNN_SAGE_U; };
template <> struct SageElem<bf16_t> { static constexpr int kVec = 8, kU = GNN_SAGE_BF16_U; };

// kArgmaxF: the argmax index stored as fp32 (exact below 2^24) -- what the SageLayer's
// torch.cat([self_feats, argmax]) promotes it to (GraphSAGE/GraphSAGE.py:17, graph_utils.py:8)
// kMaxPoolArg (the training layers, GATHER form only, with the centre half or -- gcn mode --
// without it; not a public mode number): the value
// max-pool AND its winner -- the fp32 value at the slot that wins under `beats` into out, that
// slot as a uint8 into arg_out (k <= 255). The slot is kArgmax's; the value is kMaxPool's up to
// the sign of a zero and the payload of a NaN (nanmax keeps the LAST of equal values and any
// NaN, this keeps the value AT the stored slot: the first of equal values, the first NaN).
enum SageMode : int32_t { kMean = 0, kArgmax = 1, kSum = 2, kMaxPool = 3, kArgmaxF = 4,
                          kMaxPoolArg = 5 };

// torch.max's value rule: a NaN on either side wins, else the larger value
__device__ __forceinline__ float nanmax(float a, float b) { return (a > b || a != a) ? a : b; }

template <int VW>
__device__ __forceinline__ typename Vec<VW>::T vnanmax(typename Vec<VW>::T a, typename Vec<VW>::T b) {
#pragma unroll
  for (int i = 0; i < VW; ++i) vset(a, i, nanmax(vget(a, i), vget(b, i)));
  return a;
}

// (val, idx) "a beats b" under torch.argmax's rule.
__device__ __forceinline__ bool beats(float va, int32_t ia, float vb, int32_t ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) return na && (!nb || ia < ib);
  return va > vb || (va == vb && ia < ib);
}

typedef int64_t l2 __attribute__((ext_vector_type(2)));

// SELF (gather form only): the wave also copies table[self_idx[m]] into self_out[m] -- the
// centre half of the SageLayer's cat[self, agg] (GraphSAGE/GraphSAGE.py:17, 47-48) written by
// the same launch as the aggregate half, its load in flight with the neighbour loads (a bf16
// centre row is stored widened: self_out is fp32 for every T).
// The loaded slots xv and the centre row stay as loaded (Row<T, VW>::Raw: packed bf16 pairs)
// and are widened at their use: widening at the load makes every load wait for itself.
template <typename T, int VW, int LPR, int NCH, int MODE, bool GATHER, int U, bool SELF = false>
__global__ __launch_bounds__(kSageBlock) void sage_aggregate_kernel(
    const T* __restrict__ src, int64_t ld_row, int64_t ld_m, int64_t n_table,
    const int64_t* __restrict__ idx, int64_t ldi, int64_t M, int64_t k, int64_t feat,
    void* __restrict__ out, int64_t ldo, int32_t* __restrict__ err,
    const int64_t* __restrict__ self_idx = nullptr, float* __restrict__ self_out = nullptr,
    int64_t ld_self = 0, const int64_t* __restrict__ live = nullptr,
    uint8_t* __restrict__ arg_out = nullptr, int64_t lda = 0) {
  static_assert(MODE != kMaxPoolArg || (GATHER && NCH == 1 && VW % 4 == 0),
                "the winner-recording mode exists in the GATHER vector form only");
  typedef Row<T, VW> RX;
  constexpr int EPI = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t m = static_cast<int64_t>(blockIdx.x) * kSageWaves + (threadIdx.x >> 6);
  if (m >= M || (live != nullptr && m >= *live)) return;  // live: a device row count
  const int sub = lane & (LPR - 1);
  const int grp = lane / LPR;

  typename Vec<VW>::T acc[NCH];
  int32_t arg[NCH][VW];
  typename RX::Raw self_v[NCH];
  if constexpr (SELF) {  // issued first, stored last: overlaps the neighbour gathers
    const int64_t rs = self_idx[m];
    const bool ok = rs >= 0 && rs < n_table;
    if (!ok && lane == 0) atomicOr(err, 1);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int64_t f = static_cast<int64_t>(ch * LPR + sub) * VW;
      self_v[ch] = (ok && grp == 0 && f < feat) ? RX::load(src + rs * ld_row + f) : RX::zero();
    }
  }
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    acc[ch] = (MODE == kMean || MODE == kSum) ? vzero<VW>() : typename Vec<VW>::T(-INFINITY);
#pragma unroll
    for (int i = 0; i < VW; ++i) arg[ch][i] = 0x7fffffff;
  }

  for (int64_t k0 = 0; k0 < k; k0 += EPI * U) {
    typename RX::Raw xv[U][NCH];
    int32_t kk[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = k0 + u * EPI + grp;
      kk[u] = static_cast<int32_t>(j);
      bool ok = j < k;
      const T* row = nullptr;
      if (ok) {
        if (GATHER) {
          const int64_t r = idx[m * ldi + j];
          if (r < 0 || r >= n_table) {
            ok = false;
            if (sub == 0) atomicOr(err, 1);
          } else {
            row = src + r * ld_row;
          }
        } else {
          row = src + m * ld_m + j * ld_row;
        }
      }
      if (!ok) kk[u] = 0x7fffffff;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int64_t f = static_cast<int64_t>(ch * LPR + sub) * VW;
        xv[u][ch] = (ok && f < feat) ? RX::load(row + f)
                                     : ((MODE == kMean || MODE == kSum) ? RX::zero() : RX::ninf());
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const typename Vec<VW>::T x = RX::f32(xv[u][ch]);
        if (MODE == kMean || MODE == kSum) {
          acc[ch] += x;
        } else if (MODE == kMaxPool) {
          acc[ch] = vnanmax<VW>(acc[ch], x);
        } else if (kk[u] != 0x7fffffff) {
#pragma unroll
          for (int i = 0; i < VW; ++i) {
            const float v = vget(x, i);
            if (beats(v, kk[u], vget(acc[ch], i), arg[ch][i])) {
              vset(acc[ch], i, v);
              arg[ch][i] = kk[u];
            }
          }
        }
      }
    }
  }
  // combine the EPI neighbour slots
#pragma unroll
  for (int mm = LPR; mm < kWave; mm <<= 1) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      if (MODE == kMean || MODE == kSum) {
        acc[ch] += shfl_xor_f(acc[ch], mm);
      } else if (MODE == kMaxPool) {
        acc[ch] = vnanmax<VW>(acc[ch], shfl_xor_f(acc[ch], mm));
      } else {
#pragma unroll
        for (int i = 0; i < VW; ++i) {
          const float ov = __shfl_xor(vget(acc[ch], i), mm, kWave);
          const int32_t oi = __shfl_xor(arg[ch][i], mm, kWave);
          if (beats(ov, oi, vget(acc[ch], i), arg[ch][i])) {
            vset(acc[ch], i, ov);
            arg[ch][i] = oi;
          }
        }
      }
    }
  }
  if (lane >= LPR) return;
  if constexpr (SELF) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int64_t f = static_cast<int64_t>(ch * LPR + sub) * VW;
      if (f < feat) vstore<VW>(self_out + m * ld_self + f, RX::f32(self_v[ch]));
    }
  }
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int64_t f = static_cast<int64_t>(ch * LPR + sub) * VW;
    if (f >= feat) continue;
    if (MODE == kArgmaxF) {
      typename Vec<VW>::T r;
#pragma unroll
      for (int i = 0; i < VW; ++i)
        vset(r, i, arg[ch][i] == 0x7fffffff ? 0.f : static_cast<float>(arg[ch][i]));
      vstore<VW>(static_cast<float*>(out) + m * ldo + f, r);
    } else if (MODE != kArgmax) {
      // torch.mean: sum / k;  torch.sum: the sum;  torch.max(...).values: the max
      typename Vec<VW>::T r = MODE == kMean ? acc[ch] / static_cast<float>(k) : acc[ch];
      vstore<VW>(static_cast<float*>(out) + m * ldo + f, r);
      if constexpr (MODE == kMaxPoolArg) {
        // the lane that stored VW values stores their VW winners: 4 bytes per store (no slot
        // was in range: the byte is 0)
        uint32_t* ao = reinterpret_cast<uint32_t*>(arg_out + m * lda + f);
#pragma unroll
        for (int i = 0; i < VW; i += 4) {
          uint32_t w = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b)
            w |= (arg[ch][i + b] == 0x7fffffff ? 0u : static_cast<uint32_t>(arg[ch][i + b]) & 0xffu)
                 << (8 * b);
          ao[i / 4] = w;
        }
      }
    } else {
      int64_t* o = static_cast<int64_t*>(out) + m * ldo + f;
      if constexpr (VW == 8) {  // a lane's 8 indices: four 16-B stores of two int64 each
#pragma unroll
        for (int i = 0; i < VW; i += 2)
          *reinterpret_cast<l2*>(o + i) =
              l2{arg[ch][i] == 0x7fffffff ? 0 : arg[ch][i],
                 arg[ch][i + 1] == 0x7fffffff ? 0 : arg[ch][i + 1]};
      } else {
#pragma unroll
        for (int i = 0; i < VW; ++i) o[i] = arg[ch][i] == 0x7fffffff ? 0 : arg[ch][i];
      }
    }
  }
}

template <typename T = float>
struct SageArgsT {
  const T* src;
  int64_t ld_row, ld_m, n_table;  // pitches in elements of T
  const int64_t* idx;
  int64_t ldi, M, k, feat;
  void* out;
  int64_t ldo;
  int32_t* err;
  hipStream_t s;
  const int64_t* self_idx = nullptr;  // gather form: also copy table[self_idx[m]] ...
  float* self_out = nullptr;          // ... into self_out[m] (one launch for cat[self, agg])
  int64_t ld_self = 0;
  const int64_t* live = nullptr;      // rows [0, min(*live, M)) only (device row count)
  uint8_t* arg = nullptr;             // kMaxPoolArg: the winning slot of every out[m, f]
  int64_t lda = 0;
};
typedef SageArgsT<> SageArgs;

template <int VW, int LPR, int NCH, int MODE, bool GATHER, typename T>
static int launch_sage(const SageArgsT<T>& a) {
  constexpr int U = NCH >= 2 ? 2 : SageElem<T>::kU;
  const int64_t blocks = (a.M + kSageWaves - 1) / kSageWaves;
  if (blocks > 0x7fffffffLL) return GNN_E_UNSUPPORTED;
  if (GATHER && a.self_idx != nullptr)
    hipLaunchKernelGGL((sage_aggregate_kernel<T, VW, LPR, NCH, MODE, GATHER, U, GATHER>),
                       dim3(static_cast<unsigned>(blocks)), dim3(kSageBlock), 0, a.s,
                       a.src, a.ld_row, a.ld_m, a.n_table, a.idx, a.ldi, a.M, a.k, a.feat, a.out,
                       a.ldo, a.err, a.self_idx, a.self_out, a.ld_self, a.live);
  else
    hipLaunchKernelGGL((sage_aggregate_kernel<T, VW, LPR, NCH, MODE, GATHER, U>),
                       dim3(static_cast<unsigned>(blocks)), dim3(kSageBlock), 0, a.s,
                       a.src, a.ld_row, a.ld_m, a.n_table, a.idx, a.ldi, a.M, a.k, a.feat, a.out,
                       a.ldo, a.err, nullptr, nullptr, 0, a.live);
  return launch_status();
}

template <int VW, int MODE, bool GATHER, typename T>
static int dispatch_sage(const SageArgsT<T>& a) {
  const int64_t nv = (a.feat + VW - 1) / VW;
  if (nv <= 64) {
    switch (next_pow2_le64(nv)) {
      case 1: return launch_sage<VW, 1, 1, MODE, GATHER>(a);
      case 2: return launch_sage<VW, 2, 1, MODE, GATHER>(a);
      case 4: return launch_sage<VW, 4, 1, MODE, GATHER>(a);
      case 8: return launch_sage<VW, 8, 1, MODE, GATHER>(a);
      case 16: return launch_sage<VW, 16, 1, MODE, GATHER>(a);
      case 32: return launch_sage<VW, 32, 1, MODE, GATHER>(a);
      default: return launch_sage<VW, 64, 1, MODE, GATHER>(a);
    }
  }
  if (nv <= 128) return launch_sage<VW, 64, 2, MODE, GATHER>(a);
  if (nv <= 256) return launch_sage<VW, 64, 4, MODE, GATHER>(a);
  return launch_sage<VW, 64, 8, MODE, GATHER>(a);
}

// vec: the vector path of T (SageElem<T>::kVec elements per lane), else one element per lane
template <bool GATHER, typename T>
static int run_sage(SageArgsT<T> a, int32_t mode, bool vec) {
  // feature blocks of at most 512 vectors per launch
  constexpr int VX = SageElem<T>::kVec;
  const int64_t vw = vec ? VX : 1;
  const int64_t blk = 512 * vw;
  const int64_t feat = a.feat;
  const T* src0 = a.src;
  void* out0 = a.out;
  float* self0 = a.self_out;
  for (int64_t c0 = 0; c0 < feat; c0 += blk) {
    a.feat = feat - c0 < blk ? feat - c0 : blk;
    a.src = src0 + c0;
    if (self0 != nullptr) a.self_out = self0 + c0;
    a.out = mode != kArgmax ? static_cast<void*>(static_cast<float*>(out0) + c0)
                            : static_cast<void*>(static_cast<int64_t*>(out0) + c0);
    int rc;
    if (mode == kMean)
      rc = vec ? dispatch_sage<VX, kMean, GATHER>(a) : dispatch_sage<1, kMean, GATHER>(a);
    else if (mode == kSum)
      rc = vec ? dispatch_sage<VX, kSum, GATHER>(a) : dispatch_sage<1, kSum, GATHER>(a);
    else if (mode == kMaxPool)
      rc = vec ? dispatch_sage<VX, kMaxPool, GATHER>(a) : dispatch_sage<1, kMaxPool, GATHER>(a);
    else if (mode == kArgmaxF)
      rc = vec ? dispatch_sage<VX, kArgmaxF, GATHER>(a) : dispatch_sage<1, kArgmaxF, GATHER>(a);
    else
      rc = vec ? dispatch_sage<VX, kArgmax, GATHER>(a) : dispatch_sage<1, kArgmax, GATHER>(a);
    if (rc != GNN_OK) return rc;
  }
  return GNN_OK;
}

// kMaxPoolArg: feat a power of two, one column chunk per lane (feat / kVec <= 64 lanes).
// SELF: the concat layer's form; off: the aggregate alone (the gcn-mode layer)
template <int LPR, bool SELF, typename T>
static int launch_sage_arg(const SageArgsT<T>& a) {
  constexpr int VW = SageElem<T>::kVec;
  const int64_t blocks = (a.M + kSageWaves - 1) / kSageWaves;
  if (blocks > 0x7fffffffLL) return GNN_E_UNSUPPORTED;
  hipLaunchKernelGGL(
      (sage_aggregate_kernel<T, VW, LPR, 1, kMaxPoolArg, true, SageElem<T>::kU, SELF>),
      dim3(static_cast<unsigned>(blocks)), dim3(kSageBlock), 0, a.s, a.src, a.ld_row,
      a.ld_m, a.n_table, a.idx, a.ldi, a.M, a.k, a.feat, a.out, a.ldo, a.err, a.self_idx,
      a.self_out, a.ld_self, nullptr, a.arg, a.lda);
  return launch_status();
}

template <bool SELF, typename T>
static int dispatch_sage_arg(const SageArgsT<T>& a) {
  constexpr int VX = SageElem<T>::kVec;
  switch (a.feat / VX) {
    case 1: return launch_sage_arg<1, SELF>(a);
    case 2: return launch_sage_arg<2, SELF>(a);
    case 4: return launch_sage_arg<4, SELF>(a);
    case 8: return launch_sage_arg<8, SELF>(a);
    case 16: return launch_sage_arg<16, SELF>(a);
    case 32: return launch_sage_arg<32, SELF>(a);
    default:
      if constexpr (VX == 4) return launch_sage_arg<64, SELF>(a);  // feat = 256 in fp32
      return GNN_E_UNSUPPORTED;
  }
}

// The vector path of T needs whole lanes per row (feat and every pitch of T a multiple of
// kVec, the base 16-B aligned) and fp32 / int64 outputs as the fp32 kernel's: pitch % 4 == 0,
// 16-B aligned fp32, 32-B aligned int64. Anything else runs one element per lane.
template <typename T>
static bool sage_src_vec(const T* src, int64_t feat, int64_t ld_a, int64_t ld_b) {
  constexpr int VX = SageElem<T>::kVec;
  return feat % VX == 0 && ld_a % VX == 0 && ld_b % VX == 0 && aligned_to(src, 16);
}

// ---- the C entries' bodies (gnn_sage_*_f32 in sage.hip, gnn_sage_*_bf16 in sage_bf16.hip) ----
template <typename T>
static int sage_aggregate_entry(const T* neigh, int64_t ld_k, int64_t ld_m, int64_t M, int64_t k,
                                int64_t feat, int32_t mode, void* out, int64_t ldo, void* stream) {
  if (M < 0 || k < 0 || feat < 0 || (mode < kMean || mode > kMaxPool)) return GNN_E_ARG;
  if (M == 0 || feat == 0) return GNN_OK;
  if (!neigh || !out || ld_k < feat || ldo < feat) return GNN_E_ARG;
  if (k == 0) return GNN_E_UNSUPPORTED;  // torch: mean of nothing is NaN, argmax raises
  const bool vec = sage_src_vec(neigh, feat, ld_k, ld_m) && ldo % 4 == 0 &&
                   aligned_to(out, mode != kArgmax ? 16 : 32);
  SageArgsT<T> a{neigh, ld_k, ld_m, 0, nullptr, 0, M, k, feat, out, ldo, nullptr,
                 static_cast<hipStream_t>(stream)};
  return run_sage<false>(a, mode, vec);
}

template <typename T>
static int sage_gather_aggregate_entry(const T* table, int64_t ldt, int64_t n_table,
                                       const int64_t* idx, int64_t ldi, int64_t M, int64_t k,
                                       int64_t feat, int32_t mode, void* out, int64_t ldo,
                                       int32_t* err_flag, void* stream,
                                       const int64_t* live = nullptr) {
  if (M < 0 || k < 0 || feat < 0 || n_table < 0 || (mode < kMean || mode > kMaxPool))
    return GNN_E_ARG;  // GNN_SAGE_ARGMAX_F32: the concat entries only
  if (M == 0 || feat == 0) return GNN_OK;
  if (!table || !idx || !out || !err_flag || ldt < feat || ldo < feat || ldi < k) return GNN_E_ARG;
  if (k == 0) return GNN_E_UNSUPPORTED;
  const bool vec = sage_src_vec(table, feat, ldt, 0) && ldo % 4 == 0 &&
                   aligned_to(out, mode != kArgmax ? 16 : 32);
  SageArgsT<T> a{table, ldt, 0, n_table, idx, ldi, M, k, feat, out, ldo, err_flag,
                 static_cast<hipStream_t>(stream), nullptr, nullptr, 0, live};
  return run_sage<true>(a, mode, vec);
}

// gnn_sage_gather_aggregate_live_{f32,bf16}: MEAN / MAXPOOL (the gcn-mode inference layer's
// aggregates) over rows [0, min(*live, M)) of a buffer of capacity M; live == nullptr: all M
template <typename T>
static int sage_gather_aggregate_live_entry(const T* table, int64_t ldt, int64_t n_table,
                                            const int64_t* idx, int64_t ldi, int64_t M,
                                            const int64_t* live, int64_t k, int64_t feat,
                                            int32_t mode, float* out, int64_t ldo,
                                            int32_t* err_flag, void* stream) {
  if (mode != kMean && mode != kMaxPool) return GNN_E_ARG;
  return sage_gather_aggregate_entry<T>(table, ldt, n_table, idx, ldi, M, k, feat, mode, out, ldo,
                                        err_flag, stream, live);
}

template <typename T>
static int sage_gather_concat_entry(const T* table, int64_t ldt, int64_t n_table,
                                    const int64_t* self_idx, const int64_t* idx, int64_t ldi,
                                    int64_t M, const int64_t* live, int64_t k, int64_t feat,
                                    int32_t mode, float* self_out, int64_t ld_self, float* out,
                                    int64_t ldo, int32_t* err_flag, void* stream) {
  if (M < 0 || k < 0 || feat < 0 || n_table < 0 ||
      !(mode == kMean || mode == kSum || mode == kMaxPool || mode == kArgmaxF))
    return GNN_E_ARG;
  if (M == 0 || feat == 0) return GNN_OK;
  if (!table || !self_idx || !idx || !self_out || !out || !err_flag || ldt < feat ||
      ldo < feat || ld_self < feat || ldi < k)
    return GNN_E_ARG;
  if (k == 0) return GNN_E_UNSUPPORTED;
  const bool vec = sage_src_vec(table, feat, ldt, 0) && ldo % 4 == 0 && ld_self % 4 == 0 &&
                   aligned_to(out, 16) && aligned_to(self_out, 16);
  SageArgsT<T> a{table, ldt, 0, n_table, idx, ldi, M, k, feat, out, ldo, err_flag,
                 static_cast<hipStream_t>(stream), self_idx, self_out, ld_self, live};
  return run_sage<true>(a, mode, vec);
}

// feat a power of two in [4, 256] and 1 <= k <= 255 (the slot fits a byte)
static bool sage_concat_arg_shape(int64_t feat, int64_t k) {
  return feat >= 4 && feat <= 256 && (feat & (feat - 1)) == 0 && k >= 1 && k <= 255;
}

// gnn_sage_gather_concat_arg_{f32,bf16}: MAXPOOL's cat[self, agg] plus the winning slot of every
// (row, feature) as a uint8. The vector path only: a row is whole 16-B lanes of T (so a bf16
// table needs feat >= 8: GNN_E_UNSUPPORTED), every pitch a multiple of its vector, arg in 4-B
// words (GNN_E_ALIGN otherwise).
template <typename T>
static int sage_gather_concat_arg_entry(const T* table, int64_t ldt, int64_t n_table,
                                        const int64_t* self_idx, const int64_t* idx, int64_t ldi,
                                        int64_t M, int64_t k, int64_t feat, float* self_out,
                                        int64_t ld_self, float* out, int64_t ldo, uint8_t* arg,
                                        int64_t lda, int32_t* err_flag, void* stream) {
  constexpr int VX = SageElem<T>::kVec;
  if (M < 0 || k < 0 || feat < 0 || n_table < 0) return GNN_E_ARG;
  if (!table || !self_idx || !idx || !self_out || !out || !arg || !err_flag) return GNN_E_ARG;
  if (!sage_concat_arg_shape(feat, k) || feat % VX != 0) return GNN_E_UNSUPPORTED;
  if (ldt < feat || ldo < feat || ld_self < feat || lda < feat || ldi < k) return GNN_E_ARG;
  if (ldt % VX || ldo % 4 || ld_self % 4 || lda % 4 || !aligned_to(table, 16) ||
      !aligned_to(out, 16) || !aligned_to(self_out, 16) || !aligned_to(arg, 4))
    return GNN_E_ALIGN;
  if (M == 0) return GNN_OK;
  SageArgsT<T> a{table, ldt, 0, n_table, idx, ldi, M, k, feat, out, ldo, err_flag,
                 static_cast<hipStream_t>(stream), self_idx, self_out, ld_self, nullptr, arg, lda};
  return dispatch_sage_arg<true>(a);
}

// gnn_sage_gather_aggregate_arg_{f32,bf16}: the same without the centre half (the gcn-mode
// SageLayer feeds the aggregate alone into its Linear): out[m, f] = max_j table[idx[m, j], f]
// and its winner, the rules and the shapes of the concat entry above.
template <typename T>
static int sage_gather_aggregate_arg_entry(const T* table, int64_t ldt, int64_t n_table,
                                           const int64_t* idx, int64_t ldi, int64_t M, int64_t k,
                                           int64_t feat, float* out, int64_t ldo, uint8_t* arg,
                                           int64_t lda, int32_t* err_flag, void* stream) {
  constexpr int VX = SageElem<T>::kVec;
  if (M < 0 || k < 0 || feat < 0 || n_table < 0) return GNN_E_ARG;
  if (!table || !idx || !out || !arg || !err_flag) return GNN_E_ARG;
  if (!sage_concat_arg_shape(feat, k) || feat % VX != 0) return GNN_E_UNSUPPORTED;
  if (ldt < feat || ldo < feat || lda < feat || ldi < k) return GNN_E_ARG;
  if (ldt % VX || ldo % 4 || lda % 4 || !aligned_to(table, 16) || !aligned_to(out, 16) ||
      !aligned_to(arg, 4))
    return GNN_E_ALIGN;
  if (M == 0) return GNN_OK;
  SageArgsT<T> a{table, ldt, 0, n_table, idx, ldi, M, k, feat, out, ldo, err_flag,
                 static_cast<hipStream_t>(stream), nullptr, nullptr, 0, nullptr, arg, lda};
  return dispatch_sage_arg<false>(a);
}

}  // namespace gnn
