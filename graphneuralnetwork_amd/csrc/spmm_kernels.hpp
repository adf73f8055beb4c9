// spmm_kernels.hpp -- the CSR SpMM kernels of spmm.hip / spmm_bf16.hip, generic over the
// element type of the gathered tables.
//
// XT is the element type of X, HT that of the hub table xh: float, or bf16_t (2-byte storage,
// the high half of an fp32, so the widening is exact). val, bias, the accumulators, partial
// and y are fp32 for every XT: after the load all arithmetic is the fp32 kernel's. The fp32
// instantiations live in spmm.hip, the bf16 ones in spmm_bf16.hip (see there for the lane
// layout of a bf16 row).
#pragma once

#include <type_traits>

#include "rows.hpp"

namespace gnn {

constexpr int kBlock = 256;                 // 4 waves per workgroup

// non-temporal store of one lane's VW floats
template <int VW>
__device__ __forceinline__ void nt_store(float* p, typename Vec<VW>::T v) {
  __builtin_nontemporal_store(v, reinterpret_cast<typename Vec<VW>::T*>(p));
}
template <>
__device__ __forceinline__ void nt_store<8>(float* p, f8 v) {
  __builtin_nontemporal_store(f4{v[0], v[1], v[2], v[3]}, reinterpret_cast<f4*>(p));
  __builtin_nontemporal_store(f4{v[4], v[5], v[6], v[7]}, reinterpret_cast<f4*>(p + 4));
}

#ifndef GNN_SPMM_BF16_VW
// bf16 elements per lane on the vector path: 8 = 16-B loads (a 256-B row of F = 128 on 16
// lanes, four rows per wave instruction), 4 = 8-B loads (the fp32 lane count per row, one
// reduction step fewer). A/B: tools/spmm_bf16_ab.py, DESIGN.md.
#define GNN_SPMM_BF16_VW 8
#endif
// elements per lane on the vector path, and the widest column-chunk count NCH of a launch
template <typename T> struct Elem;
template <> struct Elem<float> { static constexpr int kVec = 4; };
template <> struct Elem<bf16_t> { static constexpr int kVec = GNN_SPMM_BF16_VW; };
static_assert(GNN_SPMM_BF16_VW == 8 || GNN_SPMM_BF16_VW == 4, "bf16 lanes hold 8 or 4 elements");
constexpr int max_nch(int vw) { return vw == 8 ? 4 : 8; }  // 8 floats per chunk: 4 chunks at most

// x = bf16 with an fp32 xh (pass 2 of the XCD-sliced direct form: xh holds pass 1's fp32
// partial rows): a lane's VW elements are 2 VW bytes of an x row or 4 VW bytes of an xh row.
// Both are loaded as halves of 2 VW bytes from ONE selected pointer -- the low half always,
// the high half for an xh row only -- and kept as raw bits; which table they came from is
// decided again at the FMA (selects, no branch). Loading through a branch per table and
// widening inside it made every load wait for itself (the use sits in the branch): cfg2
// 1.22 ms against 0.89 ms for fp32 (tools/spmm_bf16_ab.py).
template <int VW> struct HalfBits;
template <> struct HalfBits<1> {
  typedef uint32_t T;
  static __device__ __forceinline__ T load(const char* p) {
    return *reinterpret_cast<const uint16_t*>(p);
  }
  static __device__ __forceinline__ T zero() { return 0u; }
};
template <> struct HalfBits<4> {
  typedef u2 T;
  static __device__ __forceinline__ T load(const char* p) { return *reinterpret_cast<const u2*>(p); }
  static __device__ __forceinline__ T zero() { return u2{0u, 0u}; }
};
template <> struct HalfBits<8> {
  typedef u4 T;
  static __device__ __forceinline__ T load(const char* p) { return *reinterpret_cast<const u4*>(p); }
  static __device__ __forceinline__ T zero() { return u4{0u, 0u, 0u, 0u}; }
};
__device__ __forceinline__ uint32_t hb_get(uint32_t v, int) { return v; }
__device__ __forceinline__ uint32_t hb_get(u2 v, int i) { return v[i]; }
__device__ __forceinline__ uint32_t hb_get(u4 v, int i) { return v[i]; }
template <int VW> struct MixedRaw {
  typename HalfBits<VW>::T lo, hi;
  // hub: the 4 VW bytes are VW floats; else lo holds VW bf16 (two per dword, or one)
  __device__ __forceinline__ typename Vec<VW>::T f32(bool hub) const {
    typename Vec<VW>::T r;
    if constexpr (VW == 1) {
      r = __uint_as_float(hub ? (lo | (hi << 16)) : (lo << 16));
    } else {
#pragma unroll
      for (int i = 0; i < VW; ++i) {
        const uint32_t fbits = i < VW / 2 ? hb_get(lo, i) : hb_get(hi, i - VW / 2);
        const uint32_t pair = hb_get(lo, i / 2);
        const uint32_t bbits = (i & 1) ? (pair & 0xffff0000u) : (pair << 16);
        vset(r, i, __uint_as_float(hub ? fbits : bbits));
      }
    }
    return r;
  }
};
// What a gather keeps in flight per neighbour row: the packed load of XT, or (kMixed) the
// raw halves above.
template <int VW, bool HUB, typename XT, typename HT> struct Fetch {
  static constexpr bool kMixed = HUB && !std::is_same<XT, HT>::value;
  static_assert(!kMixed || (sizeof(XT) == 2 && sizeof(HT) == 4), "mixed: bf16 x, fp32 xh");
  typedef Row<XT, VW> RX;
  typedef typename Vec<VW>::T V;
  typedef typename std::conditional<kMixed, MixedRaw<VW>, typename RX::Raw>::type Raw;
  static __device__ __forceinline__ Raw zero() {
    if constexpr (kMixed) return Raw{HalfBits<VW>::zero(), HalfBits<VW>::zero()};
    else return RX::zero();
  }
  // hub: the row came from xh (kMixed only)
  static __device__ __forceinline__ V f32(const Raw& r, bool hub) {
    if constexpr (kMixed) return r.f32(hub); else return RX::f32(r);
  }
};
// Fetch::kMixed only: the row of column id c (c < 0: row -1-c of xh) as a byte pointer
template <int VW, typename XT, typename HT> struct MixedRow {
  const char* p;
  bool hub;
  __device__ __forceinline__ MixedRow(const XT* x, int64_t ldx, const HT* xh, int64_t ldh, int c)
      : p(c < 0 ? reinterpret_cast<const char*>(xh + static_cast<int64_t>(-1 - c) * ldh)
                : reinterpret_cast<const char*>(x + static_cast<int64_t>(c) * ldx)),
        hub(c < 0) {}
  // elements [f, f + VW) of the row; ok: whether this lane loads at all
  __device__ __forceinline__ MixedRaw<VW> load(int64_t f, bool ok) const {
    const char* q = p + f * (hub ? 4 : 2);
    MixedRaw<VW> r;
    r.lo = ok ? HalfBits<VW>::load(q) : HalfBits<VW>::zero();
    r.hi = (ok && hub) ? HalfBits<VW>::load(q + 2 * VW) : HalfBits<VW>::zero();
    return r;
  }
};
constexpr int kWavesPerBlock = kBlock / kWave;
#ifndef GNN_SPMM_SMALL_UNROLL
// small rows per slot per wave at NCH = 1 (halved per doubling of NCH). The unrolled loads
// set the register budget of the WHOLE kernel (one launch for every row class): 16 took
// 134 VGPRs = 3 waves/SIMD, 4 takes 48 = 8 waves/SIMD. A/B with isolated variant libraries
// (tools/lib_ab.py, profiles/r02e_lib_ab_*): cfg2 1.574 -> 1.128 ms, the north star
// 18.73 -> 14.55 ms; 2 is the same, 32 spills (4x slower).
#define GNN_SPMM_SMALL_UNROLL 4
#endif
#ifndef GNN_SPMM_U
#define GNN_SPMM_U 4  // slot loads in flight per lane for one-chunk rows (A/B: tools/lib_ab.py)
#endif
#ifndef GNN_SPMM_NARROW_CH
#define GNN_SPMM_NARROW_CH 8  // edges per slot chunk in packed tasks of narrow rows (1 = LPR)
#endif
#ifndef GNN_SPMM_TASK_U
#define GNN_SPMM_TASK_U 0  // neighbour rows in flight per slot in packed tasks (0: as GNN_SPMM_U)
#endif
constexpr int kSmallUnroll = GNN_SPMM_SMALL_UNROLL;  // small rows per slot per wave (NCH = 1)
// per column-chunk count: the unrolled loads stay at ~16 x 16 B per lane
template <int NCH>
constexpr int small_unroll() {
  return kSmallUnroll / NCH >= 2 ? kSmallUnroll / NCH : 2;
}

template <typename XT = float, typename HT = XT>
struct SpmmParamsT {
  const int64_t* rowptr;
  const int32_t* col;
  const float* val;
  int64_t n_rows;
  const XT* x;
  int64_t ldx;  // in elements of XT
  int64_t feat;  // width of this column block
  const float* bias;
  float* y;
  int64_t ldy;
  int64_t seg_len;
  const int32_t* seg_row;
  const int64_t* seg_begin;
  int64_t n_seg;
  const int32_t* mid_row;  // NULL: mid rows are all rows 0..n_rows-1 (no plan)
  int64_t n_mid;
  const int32_t* small_row;
  const int32_t* small_col;
  const float* small_val;
  int64_t n_small;
  float* partial;
  int64_t ldp;
  uint32_t flags;
  // hub staging (HUB kernels): col < 0 names row -1-col of the staged hub table xh
  const HT* xh;
  int64_t ldh;  // in elements of HT
  // packed row tasks (gnn_spmm_csr_tasks_f32): task t = rows [task_row[2t], task_row[2t+1]),
  // at most kTaskRows rows, every row of degree <= the plan's packing threshold
  const int32_t* task_row;
  int64_t n_task;
  // launch geometry (wave index boundaries)
  int64_t seg_waves;
  int64_t mid_waves;
};
typedef SpmmParamsT<> SpmmParams;

// rows per packed task: the task's rowptr values (rows + 1) live in one VGPR (lane = row)
constexpr int kTaskRows = kWave - 1;

// v, the same in every lane of the wave, as a scalar (an SGPR, not a register per lane)
__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t wave_uniform(int64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<int>(v));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<int>(v >> 32));
  return static_cast<int64_t>((static_cast<uint64_t>(hi) << 32) | lo);
}

// Row ce of x -- for HUB and ce < 0, row -1-ce of xh -- seen from xs = x + the lane's offset
// in a row; dbase = xh - x in bytes, dld = ldh - ldx. The table is picked with the sign mask
// of ce, not with per-lane selects between 64-bit scalars (four moves and four selects per
// edge in a kernel that is bound by the instructions it issues).
template <bool HUB, typename XT>
__device__ __forceinline__ const XT* masked_row(const XT* xs, int64_t ldx, int64_t dbase,
                                                int64_t dld, int ce) {
  if constexpr (!HUB) {
    return xs + static_cast<int64_t>(ce) * ldx;
  } else {
    const int m = ce >> 31;  // -1: a row of xh
    const int64_t mm = m;
    const int64_t row = static_cast<uint32_t>(ce ^ m);  // ce, or -1 - ce
    // (pointer arithmetic, not integers: the loads stay global_load, not flat_load)
    const char* base = reinterpret_cast<const char*>(xs) + (mm & dbase);
    return reinterpret_cast<const XT*>(base) + row * (ldx + (mm & dld));
  }
}

// acc[ch] += sum_{e in [beg, end)} val[e] * x[col[e]][(ch*LPR + sub)*VW .. +VW)
//
// HUB: a column id c < 0 names row -1-c of the staged hub table xh (the highest-degree
// columns of X copied into one compact buffer per call, see gnn_spmm_csr_hub_f32).
template <int VW, int LPR, int NCH, int U, bool HUB = false, typename XT = float,
          typename HT = XT>
__device__ __forceinline__ void gather_rows(const int32_t* __restrict__ col,
                                            const float* __restrict__ val, int64_t beg,
                                            int64_t end, const XT* __restrict__ x,
                                            int64_t ldx, int64_t feat, int lane,
                                            typename Vec<VW>::T (&acc)[NCH],
                                            const HT* __restrict__ xh = nullptr,
                                            int64_t ldh = 0) {
  typedef Fetch<VW, HUB, XT, HT> FX;
  constexpr int EPI = kWave / LPR;
  const int sub = lane & (LPR - 1);
  const int grp = lane / LPR;
  for (int64_t base = beg; base < end; base += kWave) {
    const int n = static_cast<int>(min(static_cast<int64_t>(kWave), end - base));
    int c = 0;
    float v = 0.f;
    if (lane < n) {
      c = __builtin_nontemporal_load(col + base + lane);
      v = __builtin_nontemporal_load(val + base + lane);
    }
    for (int k = 0; k < n; k += EPI * U) {
      typename FX::Raw xv[U][NCH];
      float w[U];
      bool hubrow[FX::kMixed ? U : 1] = {};  // kMixed: which table edge u's row came from
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int e = k + u * EPI + grp;
        const int src = e & (kWave - 1);
        const int ce = __shfl(c, src, kWave);
        const float we = __shfl(v, src, kWave);
        w[u] = e < n ? we : 0.f;
        if constexpr (FX::kMixed) {
          const MixedRow<VW, XT, HT> mr(x, ldx, xh, ldh, ce);
          hubrow[u] = mr.hub;
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) {
            const int64_t f = static_cast<int64_t>(ch * LPR + sub) * VW;
            xv[u][ch] = mr.load(f, e < n && f < feat);
          }
        } else {
          const XT* xr = (HUB && ce < 0) ? xh + static_cast<int64_t>(-1 - ce) * ldh
                                         : x + static_cast<int64_t>(ce) * ldx;
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) {
            const int64_t f = static_cast<int64_t>(ch * LPR + sub) * VW;
            xv[u][ch] = (e < n && f < feat) ? FX::RX::load(xr + f) : FX::zero();
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
          acc[ch] += w[u] * FX::f32(xv[u][ch], hubrow[FX::kMixed ? u : 0]);
      }
    }
  }
}

// Combine the EPI edge slots of a wave (fixed xor-tree order: deterministic).
template <int VW, int LPR, int NCH>
__device__ __forceinline__ void reduce_slots(typename Vec<VW>::T (&acc)[NCH]) {
#pragma unroll
  for (int m = LPR; m < kWave; m <<= 1) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) acc[ch] += shfl_xor_f(acc[ch], m);
  }
}

// Epilogue for one output row held by the LPR lanes `sub` = 0..LPR-1 of a slot.
template <int VW, int LPR, int NCH, bool NT>
__device__ __forceinline__ void store_slot_row(float* __restrict__ out,
                                               const float* __restrict__ bias, int64_t feat,
                                               uint32_t flags, int sub,
                                               typename Vec<VW>::T (&acc)[NCH]) {
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int64_t f = static_cast<int64_t>(ch * LPR + sub) * VW;
    if (f >= feat) continue;
    typename Vec<VW>::T r = acc[ch];
    if (flags & GNN_EPI_ACCUMULATE) r += vload<VW>(out + f);
    if (bias != nullptr) r += vload<VW>(bias + f);
    if (flags & (GNN_EPI_RELU | GNN_EPI_ELU)) {
#pragma unroll
      for (int i = 0; i < VW; ++i) vset(r, i, act_apply(vget(r, i), flags));
    }
    if (NT)
      nt_store<VW>(out + f, r);
    else
      vstore<VW>(out + f, r);
  }
}

// The same epilogue with the lane's bias already in registers (bv; has_bias wave-uniform):
// the row write issues no load of its own unless it accumulates, so it does not have to wait
// for the gathers in flight behind which that load would queue (vmcnt retires in order).
template <int VW, int LPR, int NCH, bool NT>
__device__ __forceinline__ void store_slot_row_reg(float* __restrict__ out,
                                                   const typename Vec<VW>::T (&bv)[NCH],
                                                   bool has_bias, int64_t feat, uint32_t flags,
                                                   int sub, typename Vec<VW>::T (&acc)[NCH]) {
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int64_t f = static_cast<int64_t>(ch * LPR + sub) * VW;
    if (f >= feat) continue;
    typename Vec<VW>::T r = acc[ch];
    if (flags & GNN_EPI_ACCUMULATE) r += vload<VW>(out + f);
    if (has_bias) r += bv[ch];
    if (flags & (GNN_EPI_RELU | GNN_EPI_ELU)) {
#pragma unroll
      for (int i = 0; i < VW; ++i) vset(r, i, act_apply(vget(r, i), flags));
    }
    if (NT)
      nt_store<VW>(out + f, r);
    else
      vstore<VW>(out + f, r);
  }
}

// Rows with at most one edge, pre-resolved by the plan (small_col -1 = no edge): EPI x SU
// rows per wave, one per slot and unroll step, all SU loads issued before the stores.
template <int VW, int LPR, int NCH, bool NT, int SU, typename XT = float, typename HT = XT>
__device__ __forceinline__ void small_rows(const SpmmParamsT<XT, HT>& P, int64_t swave,
                                           int lane) {
  typedef Row<XT, VW> RX;
  constexpr int EPI = kWave / LPR;
  const int sub = lane & (LPR - 1);
  const int grp = lane / LPR;
  const int64_t i0 = swave * (EPI * SU);
  typename RX::Raw xv[SU][NCH];
  float w[SU];
  int64_t rows[SU];
#pragma unroll
  for (int u = 0; u < SU; ++u) {
    const int64_t i = i0 + u * EPI + grp;
    const bool ok = i < P.n_small;
    const int c = ok ? P.small_col[i] : -1;
    rows[u] = ok ? P.small_row[i] : -1;
    w[u] = c >= 0 ? P.small_val[i] : 0.f;
    const XT* xr = P.x + static_cast<int64_t>(c < 0 ? 0 : c) * P.ldx;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int64_t f = static_cast<int64_t>(ch * LPR + sub) * VW;
      xv[u][ch] = (c >= 0 && f < P.feat) ? RX::load(xr + f) : RX::zero();
    }
  }
#pragma unroll
  for (int u = 0; u < SU; ++u) {
    if (rows[u] < 0) continue;
    typename Vec<VW>::T r[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) r[ch] = w[u] * RX::f32(xv[u][ch]);
    store_slot_row<VW, LPR, NCH, NT>(P.y + rows[u] * P.ldy, P.bias, P.feat, P.flags, sub, r);
  }
}

// Packed row task: rows [rb, re) of consecutive ids (at most kTaskRows, each of low degree),
// their edges contiguous in col[] / val[]. The rows are split between the EPI edge slots of
// the wave by cost (edges + rows, balanced); each slot streams ITS rows' edges in CSR order,
// U neighbour rows in flight, and writes a row as soon as the stream passes its end. The
// rowptr -> col -> X dependency chain is paid once per task instead of once per row, and the
// gathers of a row overlap the bookkeeping of the next one. Each row's sum runs in edge order
// in one slot: deterministic, no shuffle reduction.
// CPL: edges per lane per chunk (a chunk = LPR * CPL edges of the slot, lane `sub` holding edges
// sub, sub + LPR, ...): narrow rows (LPR = 2 at feat 8) take several, so that a slot keeps more
// than LPR neighbour rows in flight.
template <int VW, int LPR, int NCH, int U, bool NT, bool HUB, int CPL = 1, typename XT = float,
          typename HT = XT>
__device__ __forceinline__ void packed_rows(const SpmmParamsT<XT, HT>& P, int64_t t_wave,
                                            int lane) {
  typedef Fetch<VW, HUB, XT, HT> FX;
  constexpr int EPI = kWave / LPR;
  constexpr int CH = LPR * CPL;  // edges per slot chunk
  static_assert(CH % U == 0, "a batch of U edges never straddles a chunk");
  const int sub = lane & (LPR - 1);
  const int grp = lane / LPR;
  // the task index as a scalar (the compiler cannot see that threadIdx.x >> 6 is the same in
  // every lane), so the task's rows, edge base and loop counters live in SGPRs
  const int64_t t = wave_uniform(t_wave);
  const int32_t rb = P.task_row[2 * t];
  const int32_t re = P.task_row[2 * t + 1];
  // a task outside the contract (1..kTaskRows rows inside [0, n_rows)) is skipped, never read
  // out of bounds; gnn_spmm_tasks_check reports such tasks before a launch
  if (rb < 0 || re <= rb || re - rb > kTaskRows || re > P.n_rows) return;
  const int nr = re - rb;  // 1 .. kTaskRows
  const int64_t e0 = P.rowptr[rb];
  // lane l < nr: start of row rb + l relative to e0; lanes >= nr: the task's end
  const int rp = static_cast<int>(P.rowptr[rb + min(lane, nr)] - e0);
  const int E = wave_uniform(__shfl(rp, nr, kWave));
  // slot g takes rows [sb, se): the first row whose (edges + rows) prefix reaches g/EPI of
  // the task's, found by a ballot over the row lanes
  int sb = 0, se = nr;
  if (EPI > 1) {
    const int64_t total = static_cast<int64_t>(E) + nr;
#pragma unroll
    for (int b = 1; b < EPI; ++b) {
      const int64_t target = total * b / EPI;
      const uint64_t m = __ballot(lane <= nr && static_cast<int64_t>(rp) + lane >= target);
      const int row_b = m ? (__ffsll(static_cast<unsigned long long>(m)) - 1) : nr;
      if (grp == b) sb = row_b;
      if (grp == b - 1) se = row_b;
    }
  }
  int cur = sb;                                   // the row being accumulated
  int cur_end = __shfl(rp, min(cur + 1, nr), kWave);  // its end (slot-uniform)
  // a slot that is out of rows holds kNever there, so that the test in front of every edge is
  // one compare (the last flush asks for kNever - 1: no row ends that late)
  constexpr int kNever = 0x7fffffff;
  cur_end = cur < se ? cur_end : kNever;
  const int es = __shfl(rp, sb, kWave);          // the slot's edge range [es, ee)
  const int ee = __shfl(rp, se, kWave);
  // which rows of the task have no edge, as a wave-uniform mask (bit = row). The shuffle stands
  // on its own, in front of the test of the lane: inside `lane < nr && ...` it would run with
  // the lanes >= nr masked off, and row nr - 1 reads lane nr
  const int rp_next = __shfl_down(rp, 1, kWave);
  const uint64_t empty_rows = __ballot(lane < nr && rp_next == rp);
  const bool skip_empty = (P.flags & GNN_EPI_SKIP_EMPTY) != 0;
  const uint32_t epi = P.flags & (GNN_EPI_RELU | GNN_EPI_ELU | GNN_EPI_ACCUMULATE);
  typename Vec<VW>::T acc[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) acc[ch] = vzero<VW>();
  // the lane's bias, loaded once per task (it does not change during the launch)
  typename Vec<VW>::T bv[NCH];
  const bool has_bias = P.bias != nullptr;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int64_t f = static_cast<int64_t>(ch * LPR + sub) * VW;
    bv[ch] = (has_bias && f < P.feat) ? vload<VW>(P.bias + f) : vzero<VW>();
  }

  // write every row of the slot that ends at or before edge position `pos` (several when
  // rows without edges follow each other). The only shuffle runs outside the divergent
  // branch, with the whole wave active: a ds_bpermute whose source lane (here a row index,
  // usually in another slot's lane group) is outside EXEC does not return its value.
  auto flush_upto = [&](int pos) {
    bool need = pos >= cur_end;
    while (__ballot(need)) {
      if (need) {
        const bool empty = (empty_rows >> cur) & 1;
        if (!(empty && skip_empty)) {
          float* out = P.y + static_cast<int64_t>(rb + cur) * P.ldy;
          store_slot_row_reg<VW, LPR, NCH, NT>(out, bv, has_bias, P.feat, epi, sub, acc);
        }
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) acc[ch] = vzero<VW>();
      }
      cur += need ? 1 : 0;
      const int nxt = __shfl(rp, min(cur + 1, nr), kWave);
      cur_end = need ? nxt : cur_end;
      cur_end = cur < se ? cur_end : kNever;
      need = pos >= cur_end;
    }
  };

  // what masked_row() needs (unused by the mixed instances, which widen raw halves)
  [[maybe_unused]] const XT* xs = P.x + sub * VW;
  [[maybe_unused]] const int64_t dbase =
      HUB ? reinterpret_cast<intptr_t>(P.xh) - reinterpret_cast<intptr_t>(P.x) : 0;
  [[maybe_unused]] const int64_t dld = HUB ? P.ldh - P.ldx : 0;
  // every loop below is wave-uniform (the slots' streams differ in length, so the shorter
  // ones idle with their loads masked): the shuffles read rp / c / v from any lane, and a
  // ds_bpermute from a lane outside EXEC would not return its value
  int len = ee - es;
#pragma unroll
  for (int m = 1; m < kWave; m <<= 1) len = max(len, __shfl_xor(len, m, kWave));
  len = wave_uniform(len);
  flush_upto(es);  // leading rows without edges
  for (int off = 0; off < len; off += CH) {
    const int cb = es + off;  // this slot's chunk: lane `sub` holds edges cb + sub + j * LPR
    int c[CPL];
    float v[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      c[j] = 0;
      v[j] = 0.f;
      if (cb + sub + j * LPR < ee) {
        c[j] = __builtin_nontemporal_load(P.col + e0 + cb + sub + j * LPR);
        v[j] = __builtin_nontemporal_load(P.val + e0 + cb + sub + j * LPR);
      }
    }
    const int n = min(CH, len - off);  // wave-uniform
    auto batch = [&](int k, auto kc) {  // edges k .. k + U - 1 of the chunk (kc: k when constant)
      typename FX::Raw xv[U][NCH];
      float w[U];
      bool hubrow[FX::kMixed ? U : 1] = {};
#pragma unroll
      for (int u = 0; u < U; ++u) {
        int ce;
        float we;
        if constexpr (CPL == 1) {
          const int src = grp * LPR + ((k + u) & (LPR - 1));
          ce = __shfl(c[0], src, kWave);
          we = __shfl(v[0], src, kWave);
        } else {  // k is a constant here: the register of edge k + u is known
          constexpr int K0 = decltype(kc)::value;
          const int src = grp * LPR + ((K0 + u) % LPR);
          ce = __shfl(c[(K0 + u) / LPR], src, kWave);
          we = __shfl(v[(K0 + u) / LPR], src, kWave);
        }
        const bool ok = cb + k + u < ee;
        w[u] = ok ? we : 0.f;
        if constexpr (FX::kMixed) {
          const MixedRow<VW, XT, HT> mr(P.x, P.ldx, P.xh, P.ldh, ce);
          hubrow[u] = mr.hub;
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) {
            const int64_t f = static_cast<int64_t>(ch * LPR + sub) * VW;
            xv[u][ch] = mr.load(f, ok && f < P.feat);
          }
        } else {
          const XT* xr = masked_row<HUB, XT>(xs, P.ldx, dbase, dld, ce);
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) {
            const int64_t f = static_cast<int64_t>(ch * LPR + sub) * VW;
            xv[u][ch] = (ok && f < P.feat) ? FX::RX::load(xr + ch * LPR * VW) : FX::zero();
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        flush_upto(cb + k + u);  // rows that end before this edge (all of them past ee)
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch)
          acc[ch] += w[u] * FX::f32(xv[u][ch], hubrow[FX::kMixed ? u : 0]);
      }
    };
    if constexpr (CPL == 1) {
      for (int k = 0; k < n; k += U) batch(k, std::integral_constant<int, 0>{});
    } else {  // CH / U batches, unrolled (the register index of each edge is a constant)
      static_assert(CH / U <= 4, "at most 4 batches per chunk");
      batch(0, std::integral_constant<int, 0>{});
      if constexpr (CH / U > 1) {
        if (U < n) batch(U, std::integral_constant<int, U>{});
      }
      if constexpr (CH / U > 2) {
        if (2 * U < n) batch(2 * U, std::integral_constant<int, 2 * U>{});
      }
      if constexpr (CH / U > 3) {
        if (3 * U < n) batch(3 * U, std::integral_constant<int, 3 * U>{});
      }
    }
  }
  flush_upto(kNever - 1);  // the last row and trailing rows without edges
}

template <int VW, int LPR, int NCH, int U, bool NT, bool HUB = false, bool TASKS = false,
          int CPL = 1, typename XT = float, typename HT = XT>
__global__ __launch_bounds__(kBlock) void spmm_csr_kernel(SpmmParamsT<XT, HT> P) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  const int sub = lane & (LPR - 1);
  typename Vec<VW>::T acc[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) acc[ch] = vzero<VW>();

  if (wave < P.seg_waves) {  // ---- long-row segment -> partial row
    if (wave >= P.n_seg) return;
    const int32_t row = P.seg_row[wave];
    const int64_t beg = P.seg_begin[wave];
    const int64_t end = min(beg + P.seg_len, P.rowptr[row + 1]);
    gather_rows<VW, LPR, NCH, U, HUB, XT, HT>(P.col, P.val, beg, end, P.x, P.ldx, P.feat, lane,
                                              acc, P.xh, P.ldh);
    reduce_slots<VW, LPR, NCH>(acc);
    if (lane < LPR) store_slot_row<VW, LPR, NCH, false>(P.partial + wave * P.ldp, nullptr, P.feat,
                                                        0u, sub, acc);
    return;
  }
  if (wave < P.seg_waves + P.mid_waves) {  // ---- one wave per mid row
    const int64_t i = wave - P.seg_waves;
    if (i >= P.n_mid) return;
    const int64_t row = P.mid_row ? P.mid_row[i] : i;
    gather_rows<VW, LPR, NCH, U, HUB, XT, HT>(P.col, P.val, P.rowptr[row], P.rowptr[row + 1],
                                              P.x, P.ldx, P.feat, lane, acc, P.xh, P.ldh);
    reduce_slots<VW, LPR, NCH>(acc);
    if (lane < LPR) store_slot_row<VW, LPR, NCH, NT>(P.y + row * P.ldy, P.bias, P.feat, P.flags,
                                                     sub, acc);
    return;
  }
  if constexpr (TASKS) {  // ---- packed row tasks
    const int64_t t = wave - P.seg_waves - P.mid_waves;
    if (t < P.n_task) packed_rows<VW, LPR, NCH, U, NT, HUB, CPL, XT, HT>(P, t, lane);
  } else {  // ---- packed small rows
    small_rows<VW, LPR, NCH, NT, small_unroll<NCH>(), XT, HT>(P, wave - P.seg_waves - P.mid_waves,
                                                              lane);
  }
}

// Edges per batch of spmm_items_kernel, their rows in flight at once, by lanes per row: 16 at
// LPR = 32 (F = 128), 8 at LPR = 64 (F = 256, where 16 would take 78 VGPRs and leave 6 waves
// per SIMD for a difference that cannot be told from the run-to-run spread). -DGNN_SPMM_ITEMS_U=n
// sets both (tools/spmm_items_ab.py --variants iu8,iu16; DESIGN.md sections 5.20 and 6).
constexpr int items_u(int lpr) {
#ifdef GNN_SPMM_ITEMS_U
  return GNN_SPMM_ITEMS_U;
#else
  return lpr == 32 ? 16 : 8;
#endif
}

// Plan data (rowptr, col, val) read at wave-uniform indices: through the constant address
// space such a read is a scalar load, and what it returns lives in SGPRs. The kernel never
// writes these arrays; the scalar cache is invalidated between kernels, so a caller may
// rewrite them between launches.
template <typename T>
using ConstPtr = const T __attribute__((address_space(4)))*;
template <typename T>
__device__ __forceinline__ ConstPtr<T> const_ptr(const T* p) {
  return (ConstPtr<T>)(p);
}

// acc += the K edges from e on of one item (spmm_items_kernel): the K (col, val) pairs by scalar
// loads, all K / EPI row loads issued (EPI = 64 / LPR rows per wave instruction, 16 B per lane),
// then the FMAs in edge order. With two slots (LPR = 32) the low half of the wave takes edges
// e, e + 2, ..., the high half e + 1, e + 3, ... (K is even). The two row offsets of a pair
// are scalars; a lane of the high half reaches its row by adding their difference under its
// mask hm (all ones there, zero in the low half): two ANDs instead of a 64-bit multiply per
// lane, which a select between the two column ids would leave the compiler with.
template <int LPR, int K>
__device__ __forceinline__ void items_batch(ConstPtr<int32_t> cs, ConstPtr<float> vs, int64_t e,
                                            const float* xs, uint32_t ldx, uint64_t hm, f4& acc) {
  constexpr int EPI = kWave / LPR;
  static_assert(K % EPI == 0, "whole wave instructions");
  uint32_t c[K];
  float w[K];
  f4 xv[K / EPI];
#pragma unroll
  for (int u = 0; u < K; ++u) {
    c[u] = static_cast<uint32_t>(cs[e + u]);
    w[u] = vs[e + u];
  }
#pragma unroll
  for (int j = 0; j < K / EPI; ++j) {
    uint64_t off = static_cast<uint64_t>(c[j * EPI]) * ldx;
    if constexpr (EPI == 2) off += hm & (static_cast<uint64_t>(c[j * EPI + 1]) * ldx - off);
    xv[j] = vload<4>(xs + off);
  }
#pragma unroll
  for (int j = 0; j < K / EPI; ++j) {
    float wl = w[j * EPI];
    if constexpr (EPI == 2) wl = hm ? w[j * EPI + 1] : wl;
    acc += wl * xv[j];
  }
}
// n edges from e on, n a multiple of STEP in [LO, HI]: one straight-line batch of exactly n
// edges, picked by scalar compares (a tail cut into pieces would wait for memory once per piece)
template <int LPR, int LO, int HI, int STEP>
__device__ __forceinline__ void items_tail(int n, ConstPtr<int32_t> cs, ConstPtr<float> vs,
                                           int64_t e, const float* xs, uint32_t ldx, uint64_t hm,
                                           f4& acc) {
  if constexpr (LO >= HI) {
    items_batch<LPR, LO>(cs, vs, e, xs, ldx, hm, acc);
  } else {
    constexpr int M = (LO + HI) / (2 * STEP) * STEP;  // LO <= M < HI
    if (n <= M)
      items_tail<LPR, LO, M, STEP>(n, cs, vs, e, xs, ldx, hm, acc);
    else
      items_tail<LPR, M + STEP, HI, STEP>(n, cs, vs, e, xs, ldx, hm, acc);
  }
}

// Pass 1 of the XCD-sliced direct form: part[pos] = sum_{e in item pos} val[e] * x[col[e]].
// An item is a short run of edges (2 .. the plan's chunk) whose columns are plain rows of X,
// and its partial row has no epilogue, so one wave streams the item with its edge loop in
// scalar registers: (col, val) come in by scalar loads and the 64-bit row offset col * ldx is
// scalar arithmetic. The lanes are laid out as in gather_rows, 16 B per lane: LPR = feat / 4
// lanes hold a row, so at F = 128 a wave instruction gathers two rows (edge slots) and at
// F = 256 one. Full batches of U edges, then one batch of exactly the edges that are left
// (with two slots: of the even part, then the last odd edge in the low slot alone): no lane
// predicate in the loop, and nothing is read past col[end).
//
// The sums are those of gather_rows with reduce_slots on the same item, bit for bit: slot g
// adds the edges at distance g, g + EPI, ... from the item's first edge in ascending order,
// and the row is slot 0 + slot 1.
template <int LPR, int U>
__global__ __launch_bounds__(kBlock) void spmm_items_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, int64_t n_pos, const float* __restrict__ x, uint32_t ldx,
    float* __restrict__ part, int64_t ldp) {
  constexpr int EPI = kWave / LPR;
  static_assert((LPR == 32 || LPR == 64) && U % 2 == 0, "one or two slots, whole pairs");
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane & (LPR - 1);
  const bool hi = lane >= LPR;
  // all ones in the lanes of the high slot (bit 5 of the lane spread by the shifts, so that it
  // stays a mask and the row offsets stay scalars)
  const int hbit = static_cast<int>(static_cast<uint32_t>(lane) << 26) >> 31;
  const uint64_t hm = EPI == 2 ? static_cast<uint64_t>(static_cast<int64_t>(hbit)) : 0;
  // (the compiler cannot see that threadIdx.x >> 6 is the same in every lane)
  const int64_t pos = wave_uniform(static_cast<int64_t>(blockIdx.x) * kWavesPerBlock +
                                   static_cast<int64_t>(threadIdx.x >> 6));
  if (pos >= n_pos) return;
  const ConstPtr<int64_t> rp = const_ptr(rowptr);
  const ConstPtr<int32_t> cs = const_ptr(col);
  const ConstPtr<float> vs = const_ptr(val);
  int64_t e = rp[pos];
  const int64_t end = rp[pos + 1];
  const float* xs = x + sub * 4;
  f4 acc = vzero<4>();
  for (; end - e >= U; e += U) items_batch<LPR, U>(cs, vs, e, xs, ldx, hm, acc);
  const int n = static_cast<int>(end - e);  // 0 .. U - 1
  const int whole = n & ~(EPI - 1);
  if (whole > 0) items_tail<LPR, EPI, U - EPI, EPI>(whole, cs, vs, e, xs, ldx, hm, acc);
  if constexpr (EPI == 2) {
    if (n & 1) {  // the last edge of an odd item: slot 0 only, as the masked slot of gather_rows
      const float* xr = xs + static_cast<uint64_t>(static_cast<uint32_t>(cs[end - 1])) * ldx;
      if (!hi) acc += vs[end - 1] * vload<4>(xr);
    }
    acc += shfl_xor_f(acc, LPR);
  }
  if (!hi) nt_store<4>(part + pos * ldp + sub * 4, acc);
}

// feat = 128 or 256 exactly, ldx / ldp multiples of 4, ldx < 2^32, x / part 16-B aligned:
// checked by the entry (gnn_spmm_items_f32).
template <int LPR>
static int launch_spmm_items(const int64_t* rowptr, const int32_t* col, const float* val,
                             int64_t n_pos, const float* x, int64_t ldx, float* part, int64_t ldp,
                             hipStream_t stream) {
  const int64_t blocks = (n_pos + kWavesPerBlock - 1) / kWavesPerBlock;
  if (blocks > 0x7fffffffLL) return GNN_E_UNSUPPORTED;
  hipLaunchKernelGGL((spmm_items_kernel<LPR, items_u(LPR)>), dim3(static_cast<unsigned>(blocks)),
                     dim3(kBlock), 0, stream, rowptr, col, val, n_pos, x,
                     static_cast<uint32_t>(ldx), part, ldp);
  return launch_status();
}

// y[long_row[i]] = act(sum_{s in segs(i)} partial[s] + bias).
// One workgroup (4 waves x EPI slots) per long row, UF partial-row loads in flight
// per slot, so a 1,460-segment hub row is not a serial tail; the slot / wave
// partials are combined in a fixed order (xor tree, then waves 0..3 via LDS):
// bitwise reproducible.
template <int VW, int LPR, int NCH, bool NT>
__global__ __launch_bounds__(kBlock) void spmm_fixup_kernel(
    const int32_t* __restrict__ long_row, const int32_t* __restrict__ long_seg_ptr, int64_t n_long,
    const float* __restrict__ partial, int64_t ldp, int64_t feat, const float* __restrict__ bias,
    float* __restrict__ y, int64_t ldy, uint32_t flags) {
  constexpr int EPI = kWave / LPR;
  constexpr int UF = 4;
  constexpr int STRIDE = kWavesPerBlock * EPI;
  __shared__ typename Vec<VW>::T red[kWavesPerBlock][NCH][LPR];
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x >> 6;
  const int64_t i = blockIdx.x;
  if (i >= n_long) return;
  const int sub = lane & (LPR - 1);
  const int grp = lane / LPR;
  typename Vec<VW>::T acc[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) acc[ch] = vzero<VW>();
  const int32_t s1 = long_seg_ptr[i + 1];
  for (int32_t s0 = long_seg_ptr[i] + wid * EPI + grp; s0 < s1; s0 += UF * STRIDE) {
    typename Vec<VW>::T v[UF][NCH];
#pragma unroll
    for (int u = 0; u < UF; ++u) {
      const int32_t s = s0 + u * STRIDE;
      const float* pr = partial + static_cast<int64_t>(s) * ldp;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int64_t f = static_cast<int64_t>(ch * LPR + sub) * VW;
        v[u][ch] = (s < s1 && f < feat) ? vload<VW>(pr + f) : vzero<VW>();
      }
    }
#pragma unroll
    for (int u = 0; u < UF; ++u) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) acc[ch] += v[u][ch];
    }
  }
  reduce_slots<VW, LPR, NCH>(acc);
  if (lane < LPR) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) red[wid][ch][lane] = acc[ch];
  }
  __syncthreads();
  if (wid != 0 || lane >= LPR) return;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    typename Vec<VW>::T r = red[0][ch][lane];
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) r += red[w][ch][lane];
    acc[ch] = r;
  }
  store_slot_row<VW, LPR, NCH, NT>(y + static_cast<int64_t>(long_row[i]) * ldy, bias, feat, flags,
                                   sub, acc);
}

template <typename XT = float, typename HT = XT>
struct SpmmLaunchT {
  SpmmParamsT<XT, HT> p;
  const int32_t* long_row;
  const int32_t* long_seg_ptr;
  int64_t n_long;
  hipStream_t stream;
};
typedef SpmmLaunchT<> SpmmLaunch;

template <int VW, int LPR, int NCH, bool HUB = false, typename XT = float, typename HT = XT>
static int launch_spmm_t(const SpmmLaunchT<XT, HT>& L) {
  constexpr int U = NCH >= 4 ? 1 : (NCH == 2 ? 2 : GNN_SPMM_U);
  constexpr int EPI = kWave / LPR;
  SpmmParamsT<XT, HT> p = L.p;
  const int64_t seg_blocks = (p.n_seg + kWavesPerBlock - 1) / kWavesPerBlock;
  const int64_t mid_blocks = (p.n_mid + kWavesPerBlock - 1) / kWavesPerBlock;
  if constexpr (VW == Elem<XT>::kVec) {  // the vector path of XT
    if (p.task_row != nullptr) {  // packed row tasks in place of the small-row class
      // neighbour rows in flight per slot: at most LPR (a batch never straddles a chunk of LPR
      // edges), so the narrow rows (LPR = 2: feat 5-8, 32 slots per wave) take 2
      constexpr int UT0 = (GNN_SPMM_TASK_U > 0 && NCH == 1) ? GNN_SPMM_TASK_U : (U > 1 ? U : 2);
      // rows of LPR < GNN_SPMM_NARROW_CH lanes: chunks of GNN_SPMM_NARROW_CH edges per slot,
      // all in flight at once
      constexpr int CPL = LPR < GNN_SPMM_NARROW_CH ? GNN_SPMM_NARROW_CH / LPR : 1;
      constexpr int UT = CPL > 1 ? (LPR * CPL > 8 ? 8 : LPR * CPL) : (UT0 < LPR ? UT0 : LPR);
      const int64_t task_blocks = (p.n_task + kWavesPerBlock - 1) / kWavesPerBlock;
      p.seg_waves = seg_blocks * kWavesPerBlock;
      p.mid_waves = mid_blocks * kWavesPerBlock;
      const int64_t blocks = seg_blocks + mid_blocks + task_blocks;
      if (blocks > 0x7fffffffLL) return GNN_E_UNSUPPORTED;
      if (blocks > 0)
        hipLaunchKernelGGL((spmm_csr_kernel<VW, LPR, NCH, UT, true, HUB, true, CPL, XT, HT>),
                           dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, L.stream, p);
      if (L.n_long > 0)
        hipLaunchKernelGGL((spmm_fixup_kernel<VW, LPR, NCH, true>), dim3(static_cast<unsigned>(L.n_long)),
                           dim3(kBlock), 0, L.stream, L.long_row, L.long_seg_ptr, L.n_long, p.partial,
                           p.ldp, p.feat, p.bias, p.y, p.ldy, p.flags & ~GNN_EPI_SKIP_EMPTY);
      return launch_status();
    }
  }
  if (p.task_row != nullptr) return GNN_E_UNSUPPORTED;
  constexpr int SU = small_unroll<NCH>();
  const int64_t small_waves = (p.n_small + EPI * SU - 1) / (EPI * SU);
  const int64_t small_blocks = (small_waves + kWavesPerBlock - 1) / kWavesPerBlock;
  p.seg_waves = seg_blocks * kWavesPerBlock;
  p.mid_waves = mid_blocks * kWavesPerBlock;
  const int64_t blocks = seg_blocks + mid_blocks + small_blocks;
  if (blocks > 0x7fffffffLL) return GNN_E_UNSUPPORTED;
  if (blocks > 0) {
    hipLaunchKernelGGL((spmm_csr_kernel<VW, LPR, NCH, U, true, HUB, false, 1, XT, HT>),
                       dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, L.stream, p);
  }
  if (L.n_long > 0) {
    hipLaunchKernelGGL((spmm_fixup_kernel<VW, LPR, NCH, true>), dim3(static_cast<unsigned>(L.n_long)),
                       dim3(kBlock), 0, L.stream, L.long_row, L.long_seg_ptr, L.n_long, p.partial,
                       p.ldp, p.feat, p.bias, p.y, p.ldy, p.flags);
  }
  return launch_status();
}

template <int VW, int LPR, int NCH, typename XT = float, typename HT = XT>
static int launch_spmm(const SpmmLaunchT<XT, HT>& L) {
  // two element types: only the hub form exists (spmm_entry never gets here without xh)
  if constexpr (!std::is_same<XT, HT>::value)
    return L.p.xh ? launch_spmm_t<VW, LPR, NCH, true, XT, HT>(L) : GNN_E_ARG;
  else
    return L.p.xh ? launch_spmm_t<VW, LPR, NCH, true, XT, HT>(L)
                  : launch_spmm_t<VW, LPR, NCH, false, XT, HT>(L);
}

// Picks (VW, LPR, NCH) for one column block of width feat (<= 64 * max_nch(VW) * VW).
template <int VW, typename XT = float, typename HT = XT>
static int dispatch_spmm(const SpmmLaunchT<XT, HT>& L) {
  const int64_t nv = (L.p.feat + VW - 1) / VW;  // vectors per row
  if (nv <= 64) {
    switch (next_pow2_le64(nv)) {
      case 1: return launch_spmm<VW, 1, 1, XT, HT>(L);
      case 2: return launch_spmm<VW, 2, 1, XT, HT>(L);
      case 4: return launch_spmm<VW, 4, 1, XT, HT>(L);
      case 8: return launch_spmm<VW, 8, 1, XT, HT>(L);
      case 16: return launch_spmm<VW, 16, 1, XT, HT>(L);
      case 32: return launch_spmm<VW, 32, 1, XT, HT>(L);
      default: return launch_spmm<VW, 64, 1, XT, HT>(L);
    }
  }
  if (nv <= 128) return launch_spmm<VW, 64, 2, XT, HT>(L);
  if (nv <= 256) return launch_spmm<VW, 64, 4, XT, HT>(L);
  if constexpr (max_nch(VW) >= 8)
    return launch_spmm<VW, 64, 8, XT, HT>(L);
  else
    return GNN_E_UNSUPPORTED;  // run_spmm cuts narrower column blocks
}

static int check_spmm_args(const int64_t* rowptr, int64_t n_rows, const void* x, int64_t ldx,
                           int64_t feat, float* y, int64_t ldy, int64_t seg_len, int64_t n_seg,
                           int64_t n_long, int64_t n_small, int64_t n_mid, const int32_t* seg_row,
                           const int64_t* seg_begin, const int32_t* long_row,
                           const int32_t* long_seg_ptr, const int32_t* small_row,
                           const int32_t* small_col, const float* small_val,
                           const int32_t* mid_row, const float* partial, uint32_t flags) {
  if (n_rows < 0 || feat < 0 || n_seg < 0 || n_long < 0 || n_small < 0 || seg_len < 1)
    return GNN_E_ARG;
  if (rowptr == nullptr || y == nullptr || x == nullptr) return GNN_E_ARG;
  if (ldx < feat || ldy < feat) return GNN_E_ARG;
  if (n_rows > 0x7fffffffLL) return GNN_E_UNSUPPORTED;  // int32 column ids / row lists
  if ((n_seg > 0 || n_long > 0) &&
      (seg_row == nullptr || seg_begin == nullptr || long_row == nullptr ||
       long_seg_ptr == nullptr || partial == nullptr || n_long == 0 || n_seg == 0))
    return GNN_E_ARG;
  if (n_small > 0 && (small_row == nullptr || small_col == nullptr || small_val == nullptr))
    return GNN_E_ARG;
  if (mid_row != nullptr && (n_mid < 0 || n_mid + n_small + n_long > n_rows)) return GNN_E_ARG;
  if (flags & ~(GNN_EPI_RELU | GNN_EPI_ELU | GNN_EPI_ACCUMULATE | GNN_EPI_SKIP_EMPTY))
    return GNN_E_ARG;
  return GNN_OK;
}

// The vector path of XT (VX = Elem<XT>::kVec elements per lane: fp32 x 4 or bf16 x 8 in 16 B,
// bf16 x 4 in 8 B) needs whole lanes per row, lane-aligned tables and 16-B aligned fp32
// operands; everything else (odd widths, views off by one element, odd row pitch) runs the
// one-element-per-lane path.
template <typename XT, typename HT>
static bool spmm_vector_ok(const SpmmLaunchT<XT, HT>& L, const XT* x, const float* bias,
                           const float* y, const float* partial, int64_t feat) {
  constexpr int VX = Elem<XT>::kVec;
  constexpr int VH = sizeof(HT) == 4 ? 4 : VX;  // fp32 xh rows: 16-B pieces
  const HT* xh = L.p.xh;
  return (feat % VX == 0) && (L.p.ldx % VX == 0) && (L.p.ldy % 4 == 0) &&
         aligned_to(x, VX * sizeof(XT)) && aligned_to(y, 16) &&
         (xh == nullptr || (aligned_to(xh, VH * sizeof(HT)) && L.p.ldh % VH == 0)) &&
         (bias == nullptr || aligned_to(bias, 16)) &&
         (partial == nullptr || aligned_to(partial, 16));
}

template <typename XT, typename HT>
static int run_spmm(SpmmLaunchT<XT, HT> L, const XT* x, const float* bias, float* y,
                    float* partial, int64_t feat) {
  constexpr int VX = Elem<XT>::kVec;
  const HT* xh = L.p.xh;
  const bool vec4 = spmm_vector_ok(L, x, bias, y, partial, feat);
  const int64_t vw = vec4 ? VX : 1;
  const int64_t blk = 64 * max_nch(vw) * vw;  // widest column block one launch covers
  for (int64_t c0 = 0; c0 < feat; c0 += blk) {
    L.p.feat = feat - c0 < blk ? feat - c0 : blk;
    L.p.x = x + c0;
    L.p.xh = xh ? xh + c0 : nullptr;
    L.p.y = y + c0;
    L.p.bias = bias ? bias + c0 : nullptr;
    L.p.partial = partial ? partial + c0 : nullptr;
    const int rc = vec4 ? dispatch_spmm<VX, XT, HT>(L) : dispatch_spmm<1, XT, HT>(L);
    if (rc != GNN_OK) return rc;
  }
  return GNN_OK;
}

template <typename XT = float, typename HT = XT>
static int spmm_entry(const int64_t* rowptr, const int32_t* col, const float* val, int64_t n_rows,
                      const XT* x, int64_t ldx, int64_t feat, const float* bias, float* y,
                      int64_t ldy, int64_t seg_len, const int32_t* seg_row,
                      const int64_t* seg_begin, int64_t n_seg, const int32_t* long_row,
                      const int32_t* long_seg_ptr, int64_t n_long, const int32_t* small_row,
                      const int32_t* small_col, const float* small_val, int64_t n_small,
                      const int32_t* mid_row, int64_t n_mid, float* partial, uint32_t flags,
                      void* stream, const HT* xh = nullptr, int64_t ldh = 0,
                      const int32_t* task_row = nullptr, int64_t n_task = 0) {
  int rc = check_spmm_args(rowptr, n_rows, x, ldx, feat, y, ldy, seg_len, n_seg, n_long, n_small,
                           n_mid, seg_row, seg_begin, long_row, long_seg_ptr, small_row, small_col,
                           small_val, mid_row, partial, flags);
  if (rc != GNN_OK) return rc;
  if (xh != nullptr && ldh < feat) return GNN_E_ARG;
  if (xh == nullptr && !std::is_same<XT, HT>::value) return GNN_E_ARG;
  if (n_rows == 0 || feat == 0) return GNN_OK;
  const bool plan = mid_row != nullptr;
  SpmmLaunchT<XT, HT> L{};
  L.p.rowptr = rowptr;
  L.p.col = col;
  L.p.val = val;
  L.p.n_rows = n_rows;
  L.p.ldx = ldx;
  L.p.ldy = ldy;
  L.p.seg_len = plan ? seg_len : INT64_MAX;  // no plan: every row by one wave
  L.p.seg_row = seg_row;
  L.p.seg_begin = seg_begin;
  L.p.n_seg = plan ? n_seg : 0;
  L.p.mid_row = mid_row;
  L.p.n_mid = plan ? n_mid : n_rows;
  L.p.small_row = small_row;
  L.p.small_col = small_col;
  L.p.small_val = small_val;
  L.p.n_small = plan ? n_small : 0;
  L.p.ldp = feat;
  L.p.flags = flags;
  L.p.xh = xh;
  L.p.ldh = ldh;
  L.p.task_row = task_row;
  L.p.n_task = n_task;
  L.long_row = long_row;
  L.long_seg_ptr = long_seg_ptr;
  L.n_long = plan ? n_long : 0;
  L.stream = static_cast<hipStream_t>(stream);
  return run_spmm(L, x, bias, y, partial, feat);
}

}  // namespace gnn
