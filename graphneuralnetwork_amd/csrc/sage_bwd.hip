// sage_bwd.hip -- the backward of the GraphSAGE training layer on gfx950: the adjoint of
// gnn_sage_gather_concat_f32 in MEAN mode (sage_kernels.hpp, SELF form).
//
// Forward, per output row m of a layer (GraphSAGE/GraphSAGE.py:17, 47-49, graph_utils.py:6):
//   buf[m, 0:F]  = X[cidx[m]]                      (the centre row)
//   buf[m, F:2F] = (1/k) sum_j X[idx[m, j]]        (the neighbour mean)
// so the gradient of X gathers rows of dBuf through the TRANSPOSED maps:
//   dX[t] = sum_{m: cidx[m] = t} dBuf[m, 0:F] + (1/k) sum_{(m, j): idx[m, j] = t} dBuf[m, F:2F].
//
// The M (k + 1) contributions are numbered as slots: slot s < M is centre row s, slot s >= M
// is neighbour entry e = s - M (row e / k, column e % k).
//
//   gnn_sage_maps_transpose: ptr / slot, the slots of every target t in ascending slot order
//     (a stable radix sort of the slots by target, rocPRIM, then one lower bound per target),
//     so the summation order below is a function of the maps alone.
//   gnn_sage_scatter_concat_f32: one lane group of F/4 lanes per target walks its slot list in
//     order (16-B loads, kSbU gradient rows in flight, fp32 adds). A list longer than kSbChunk
//     slots (a hub drawn by thousands of seeds) is cut into chunks of kSbChunk: one wavefront
//     per chunk writes a partial row, and a last pass adds the partial rows of a target in
//     chunk order. No floating-point atomics anywhere; the integer atomics only hand out
//     places in the chunk list, and no sum depends on the place it was given.
//   gnn_sage_scatter_concat_maxpool_f32: the same three passes for the MAXPOOL layer
//     (gnn_sage_gather_concat_arg_f32 / _bf16), whose aggregate half is
//     buf[m, F + f] = X[idx[m, arg[m, f]], f]: a neighbour slot (m, j) contributes
//     dBuf[m, F + f] where arg[m, f] == j and nothing elsewhere (a select, so a NaN or Inf
//     gradient of a slot that did not win reaches nobody), unscaled. The kernels are the MEAN
//     ones instantiated over SbMaskArgs; the MEAN instances take SbArgs as before.
//   gnn_sage_maps_transpose_nbr, gnn_sage_scatter_agg_f32 / _maxpool_f32: the same for the
//     gcn-mode layer (GraphSAGE/GraphSAGE.py:13-14: buf[m] = agg_j X[idx[m, j]], no centre half):
//     M k slots, slot e the entry (e / k, e % k), dBuf [M, F]. The slot decoding is a property of
//     the argument struct (SbAggArgs / SbAggMaskArgs); the passes are the ones above.
#include <cstring>  // rocprim's texture_cache_iterator calls host memset

#include <rocprim/rocprim.hpp>

#include "common.hpp"
#include "host.hpp"

namespace gnn {

constexpr int kSbBlock = 256;
constexpr int kSbWaves = kSbBlock / kWave;
#ifndef GNN_SB_CHUNK
#define GNN_SB_CHUNK 256  // slots per chunk of a split list
#endif
#ifndef GNN_SB_U
#define GNN_SB_U 4        // gradient rows in flight per lane group
#endif
constexpr int kSbChunk = GNN_SB_CHUNK;
constexpr int kSbU = GNN_SB_U;
constexpr int kSbGrid = 2048;  // the chunk / combine passes: a fixed grid, sizes read on the device

// The slots of a layer, or -1 where they do not fit an int32 slot id. CENTRE: M (k + 1); off
// (the gcn-mode layer has no centre half): M k, slot e is entry (e / k, e % k)
template <bool CENTRE>
static int64_t sb_slots(int64_t M, int64_t k) {
  const int64_t per_row = CENTRE ? k + 1 : k;
  if (per_row > 0 && M > 0x7fffffffLL / per_row) return -1;
  return M * per_row;
}

static unsigned sb_key_bits(int64_t n_prev) {  // keys are targets in [0, n_prev]
  unsigned b = 1;
  while (b < 32 && (1LL << b) <= n_prev) ++b;
  return b;
}

static size_t sb_sort_temp(int64_t n, unsigned bits) {
  size_t t = 0;
  (void)rocprim::radix_sort_pairs(nullptr, t, static_cast<uint32_t*>(nullptr),
                                  static_cast<uint32_t*>(nullptr),
                                  rocprim::counting_iterator<int32_t>(0),
                                  static_cast<int32_t*>(nullptr), static_cast<size_t>(n), 0, bits);
  return t;
}

// keys[s] = the target of slot s; an index outside [0, n_prev) raises the flag and sorts last
// (key n_prev), past ptr[n_prev]: the scatter never reads its slot.
// CENTRE: the M centre slots come first (the concat layer); off: the neighbour map alone
template <bool CENTRE>
__global__ __launch_bounds__(kSbBlock) void sage_slot_keys_kernel(
    const int64_t* __restrict__ cidx, const int64_t* __restrict__ idx, int64_t ldi, int64_t M,
    int64_t k, int64_t n_prev, uint32_t* __restrict__ keys, int32_t* __restrict__ err) {
  const int64_t n = M * (CENTRE ? k + 1 : k);
  const int64_t step = static_cast<int64_t>(gridDim.x) * kSbBlock;
  for (int64_t s = static_cast<int64_t>(blockIdx.x) * kSbBlock + threadIdx.x; s < n; s += step) {
    int64_t t;
    if (CENTRE && s < M) {
      t = cidx[s];
    } else {
      const uint32_t e = static_cast<uint32_t>(CENTRE ? s - M : s), kk = static_cast<uint32_t>(k);
      t = idx[static_cast<int64_t>(e / kk) * ldi + e % kk];
    }
    if (t < 0 || t >= n_prev) {
      atomicOr(err, 1);
      t = n_prev;
    }
    keys[s] = static_cast<uint32_t>(t);
  }
}

// ptr[t] = the first position of the sorted keys holding a key >= t, t in [0, n_prev]
__global__ __launch_bounds__(kSbBlock) void sage_slot_ptr_kernel(
    const uint32_t* __restrict__ keys, int64_t n, int64_t n_prev, int64_t* __restrict__ ptr) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kSbBlock + threadIdx.x;
  if (t > n_prev) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (static_cast<int64_t>(keys[mid]) < t) lo = mid + 1;
    else hi = mid;
  }
  ptr[t] = lo;
}

struct SbArgs {
  const float* dbuf;
  int64_t ldd;
  const int64_t* ptr;
  const int32_t* slot;
  int64_t M, k, n_prev, n_slots;
  float inv_k;
  float* dx;
  int64_t ldx;
  int32_t* count;  // [0] chunks handed out, [1] split targets
  int2* longs;     // (target, first chunk) of every split target
  int2* tasks;     // (target, chunk number) of every chunk
  float* part;     // one partial row per chunk
  int32_t max_long, max_tasks;
  // how a slot is decoded. kCentre: slots [0, M) are centre rows (dbuf[s, 0:F], unscaled), the
  // neighbour entries follow and read dbuf[m, F:2F]; off (the gcn-mode layer, SbAgg*Args):
  // every slot is a neighbour entry e = (m, j) and reads dbuf[m, 0:F]. kMask: the MAXPOOL select
  static constexpr bool kCentre = true, kMask = false;
};

// MAXPOOL: arg[m, f] (uint8, pitch lda) is the neighbour column whose row won feature f of row m
struct SbMaskArgs : SbArgs {
  const uint8_t* arg;
  int64_t lda;
  static constexpr bool kMask = true;
};

// the gcn-mode layer (gnn_sage_scatter_agg_f32 / _maxpool_f32): no centre slots, dbuf is [M, F]
struct SbAggArgs : SbArgs {
  static constexpr bool kCentre = false;
};
struct SbAggMaskArgs : SbMaskArgs {
  static constexpr bool kCentre = false;
};

// The masked sum of sb_sum below: a centre slot adds its row, a neighbour slot (m, j) the
// elements of dbuf[m, F:2F] whose arg byte is j. Each lane loads the 4 bytes of
// arg[m, 4 sub : 4 sub + 4] beside its 16-B gradient load; the mask SELECTS (x or 0.f), it
// never multiplies.
template <bool CENTRE>
__device__ __forceinline__ f4 sb_sum_mask(const SbMaskArgs& a, int64_t b, int64_t e, int64_t step,
                                          int F, int sub) {
  f4 acc = vzero<4>();
  const uint32_t m32 = static_cast<uint32_t>(a.M), k32 = static_cast<uint32_t>(a.k);
  constexpr uint32_t kAll = 0x100;  // no byte equals it: a centre slot keeps every element
  for (int64_t p = b; p < e; p += step * kSbU) {
    f4 v[kSbU];
    uint32_t win[kSbU], col[kSbU];
#pragma unroll
    for (int u = 0; u < kSbU; ++u) {
      v[u] = vzero<4>();
      win[u] = 0;
      col[u] = kAll;
      const int64_t q = p + u * step;
      if (q < e) {
        const uint32_t s = static_cast<uint32_t>(a.slot[q]);
        if (s < static_cast<uint32_t>(a.n_slots)) {
          const float* row;
          if (CENTRE && s < m32) {
            row = a.dbuf + static_cast<int64_t>(s) * a.ldd;
          } else {
            const uint32_t en = CENTRE ? s - m32 : s;
            const uint32_t m = en / k32;
            row = a.dbuf + static_cast<int64_t>(m) * a.ldd + (CENTRE ? F : 0);
            col[u] = en - m * k32;
            win[u] = *reinterpret_cast<const uint32_t*>(a.arg + static_cast<int64_t>(m) * a.lda +
                                                        4 * sub);
          }
          v[u] = vload<4>(row + 4 * sub);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kSbU; ++u) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool keep = col[u] == kAll || ((win[u] >> (8 * i)) & 0xffu) == col[u];
        vset(acc, i, vget(acc, i) + (keep ? vget(v[u], i) : 0.f));
      }
    }
  }
  return acc;
}

// The sum over the slots at positions b, b + step, ... < e of the sorted list, in that order,
// by one lane group: lane `sub` holds floats [4 sub, 4 sub + 4) of the row; kSbU loads in flight.
// A slot outside [0, n_slots) (no builder writes one) contributes nothing.
template <bool CENTRE>
__device__ __forceinline__ f4 sb_sum_mean(const SbArgs& a, int64_t b, int64_t e, int64_t step,
                                          int F, int sub) {
  f4 acc = vzero<4>();
  const uint32_t m32 = static_cast<uint32_t>(a.M), k32 = static_cast<uint32_t>(a.k);
  for (int64_t p = b; p < e; p += step * kSbU) {
    f4 v[kSbU];
    float sc[kSbU];
#pragma unroll
    for (int u = 0; u < kSbU; ++u) {
      v[u] = vzero<4>();
      sc[u] = 1.f;
      const int64_t q = p + u * step;
      if (q < e) {
        const uint32_t s = static_cast<uint32_t>(a.slot[q]);
        if (s < static_cast<uint32_t>(a.n_slots)) {
          const float* row;
          if (CENTRE && s < m32) {
            row = a.dbuf + static_cast<int64_t>(s) * a.ldd;
          } else {
            row = a.dbuf + static_cast<int64_t>((CENTRE ? s - m32 : s) / k32) * a.ldd +
                  (CENTRE ? F : 0);
            sc[u] = a.inv_k;
          }
          v[u] = vload<4>(row + 4 * sub);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kSbU; ++u) acc += v[u] * sc[u];
  }
  return acc;
}

// the sum of an argument struct: its slot decoding (kCentre) and its select (kMask)
template <typename A>
__device__ __forceinline__ f4 sb_sum(const A& a, int64_t b, int64_t e, int64_t step, int F,
                                     int sub) {
  if constexpr (A::kMask) return sb_sum_mask<A::kCentre>(a, b, e, step, F, sub);
  else return sb_sum_mean<A::kCentre>(a, b, e, step, F, sub);
}

// the slot range of target t, empty unless it lies inside the slot array
__device__ __forceinline__ void sb_range(const SbArgs& a, int64_t t, int64_t& b, int64_t& e) {
  b = a.ptr[t];
  e = a.ptr[t + 1];
  if (b < 0 || e > a.n_slots || b > e) b = e = 0;
}

// pass 1: one lane group per target. Lists of at most kSbChunk slots are summed and stored
// (an empty list stores zeros: the kernel owns all of dx); a longer one is entered into the
// chunk list and left to passes 2 and 3.
template <int LPR, typename A = SbArgs>
__global__ __launch_bounds__(kSbBlock) void sage_scatter_rows_kernel(A a) {
  constexpr int F = 4 * LPR;
  const int64_t t = (static_cast<int64_t>(blockIdx.x) * kSbBlock + threadIdx.x) / LPR;
  const int sub = threadIdx.x % LPR;
  if (t >= a.n_prev) return;
  int64_t b, e;
  sb_range(a, t, b, e);
  if (e - b > kSbChunk) {
    if (sub == 0) {
      const int32_t nc = static_cast<int32_t>((e - b + kSbChunk - 1) / kSbChunk);
      const int32_t base = atomicAdd(a.count, nc);
      const int32_t li = atomicAdd(a.count + 1, 1);
      if (li < a.max_long && base >= 0 && base <= a.max_tasks - nc) {
        a.longs[li] = make_int2(static_cast<int32_t>(t), base);
        for (int32_t c = 0; c < nc; ++c) a.tasks[base + c] = make_int2(static_cast<int32_t>(t), c);
      }
    }
    return;
  }
  vstore<4>(a.dx + t * a.ldx + 4 * sub, sb_sum(a, b, e, 1, F, sub));
}

// pass 2: one wavefront per chunk. Its 64 / LPR lane groups take the chunk's slots round robin
// (each in ascending order), the group sums are added by xor-shuffles: a fixed tree.
template <int LPR, typename A = SbArgs>
__global__ __launch_bounds__(kSbBlock) void sage_scatter_chunks_kernel(A a) {
  constexpr int F = 4 * LPR;
  constexpr int EPI = kWave / LPR;
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane % LPR, grp = lane / LPR;
  int32_t n_task = a.count[0];
  if (n_task > a.max_tasks) n_task = a.max_tasks;
  const int32_t nw = gridDim.x * kSbWaves;
  for (int32_t p = blockIdx.x * kSbWaves + (threadIdx.x >> 6); p < n_task; p += nw) {
    const int2 tk = a.tasks[p];
    f4 acc = vzero<4>();
    if (tk.x >= 0 && tk.x < a.n_prev && tk.y >= 0) {
      int64_t b, e;
      sb_range(a, tk.x, b, e);
      b += static_cast<int64_t>(tk.y) * kSbChunk;
      if (e > b + kSbChunk) e = b + kSbChunk;
      acc = sb_sum(a, b + grp, e, EPI, F, sub);
    }
#pragma unroll
    for (int mm = LPR; mm < kWave; mm <<= 1) acc += shfl_xor_f(acc, mm);
    if (lane < LPR) vstore<4>(a.part + static_cast<int64_t>(p) * F + 4 * sub, acc);
  }
}

// pass 3: one lane group per split target adds its partial rows in chunk order (the partial
// rows are already masked: MAXPOOL runs the same instance)
template <int LPR>
__global__ __launch_bounds__(kSbBlock) void sage_scatter_combine_kernel(SbArgs a) {
  constexpr int F = 4 * LPR;
  const int sub = threadIdx.x % LPR;
  int32_t n_long = a.count[1];
  if (n_long > a.max_long) n_long = a.max_long;
  const int32_t ng = gridDim.x * (kSbBlock / LPR);
  for (int32_t i = (blockIdx.x * kSbBlock + threadIdx.x) / LPR; i < n_long; i += ng) {
    const int2 lg = a.longs[i];
    if (lg.x < 0 || lg.x >= a.n_prev) continue;
    int64_t b, e;
    sb_range(a, lg.x, b, e);
    const int64_t nc = (e - b + kSbChunk - 1) / kSbChunk;
    if (lg.y < 0 || lg.y > a.max_tasks - nc) continue;
    f4 acc = vzero<4>();
    for (int64_t c = 0; c < nc; c += kSbU) {
      f4 v[kSbU];
#pragma unroll
      for (int u = 0; u < kSbU; ++u)
        v[u] = c + u < nc ? vload<4>(a.part + (lg.y + c + u) * F + 4 * sub) : vzero<4>();
#pragma unroll
      for (int u = 0; u < kSbU; ++u) acc += v[u];
    }
    vstore<4>(a.dx + static_cast<int64_t>(lg.x) * a.ldx + 4 * sub, acc);
  }
}

template <int LPR, typename A>
static int launch_sage_scatter(const A& a, hipStream_t s) {
  const int64_t blocks = (a.n_prev * LPR + kSbBlock - 1) / kSbBlock;
  if (blocks > 0x7fffffffLL) return GNN_E_UNSUPPORTED;
  GNN_TRY(hipMemsetAsync(a.count, 0, 2 * sizeof(int32_t), s));
  hipLaunchKernelGGL((sage_scatter_rows_kernel<LPR, A>), dim3(static_cast<unsigned>(blocks)),
                     dim3(kSbBlock), 0, s, a);
  int64_t g = (static_cast<int64_t>(a.max_tasks) + kSbWaves - 1) / kSbWaves;
  g = g < kSbGrid ? g : kSbGrid;
  hipLaunchKernelGGL((sage_scatter_chunks_kernel<LPR, A>), dim3(static_cast<unsigned>(g)),
                     dim3(kSbBlock), 0, s, a);
  g = (static_cast<int64_t>(a.max_long) * LPR + kSbBlock - 1) / kSbBlock;
  g = g < kSbGrid ? g : kSbGrid;
  hipLaunchKernelGGL((sage_scatter_combine_kernel<LPR>), dim3(static_cast<unsigned>(g)),
                     dim3(kSbBlock), 0, s, static_cast<const SbArgs&>(a));
  return launch_status();
}

// the workspace of the scatter: counters | split targets | chunks | partial rows
struct SbWs {
  int32_t* count;  // SbArgs' pieces
  int2* longs;
  int2* tasks;
  float* part;
  int32_t max_long, max_tasks;  // n_slots fits an int32
  int64_t bytes;
};
static SbWs sb_carve(void* ws, int64_t n_slots, int64_t F) {
  Carve c{static_cast<char*>(ws)};
  SbWs w{};
  // every split list holds more than kSbChunk slots; sum of ceil(len / chunk) <= n / chunk + lists
  w.max_long = static_cast<int32_t>(n_slots / kSbChunk + 1);
  w.max_tasks = static_cast<int32_t>(2 * (n_slots / kSbChunk) + 2);
  w.count = c.take<int32_t>(2);
  w.longs = c.take<int2>(w.max_long);
  w.tasks = c.take<int2>(w.max_tasks);
  w.part = c.take<float>(w.max_tasks * F);
  w.bytes = c.used;
  return w;
}

// the workspace of a transpose over n slots: keys | sorted keys | rocPRIM's temporary, sized
// for 32-bit keys
struct SbTransposeWs {
  uint32_t* k0;
  uint32_t* k1;
  void* temp;
  size_t temp_bytes;
  int64_t bytes;
};
static SbTransposeWs sb_transpose_carve(void* ws, int64_t n) {
  Carve c{static_cast<char*>(ws)};
  SbTransposeWs w{};
  w.k0 = c.take<uint32_t>(n);
  w.k1 = c.take<uint32_t>(n);
  w.temp_bytes = sb_sort_temp(n > 0 ? n : 1, 32);
  w.temp = c.raw(static_cast<int64_t>(w.temp_bytes));
  c.raw(1 << 20);
  w.bytes = c.used;
  return w;
}

}  // namespace gnn

using namespace gnn;

// the body of both transposes: the arguments are checked, n = the number of slots
template <bool CENTRE>
static int sb_transpose(const int64_t* cidx, const int64_t* idx, int64_t ldi, int64_t M, int64_t k,
                        int64_t n_prev, int64_t n, int64_t* ptr, int32_t* slot, int32_t* err_flag,
                        void* workspace, int64_t workspace_bytes, void* stream) {
  const SbTransposeWs w = sb_transpose_carve(workspace, n);
  if (workspace_bytes < w.bytes) return GNN_E_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n > 0) {
    // the temporary of this call's key width must fit what follows the keys
    const unsigned bits = sb_key_bits(n_prev);
    size_t tb = sb_sort_temp(n, bits);
    const int64_t room = workspace_bytes - (static_cast<char*>(w.temp) - static_cast<char*>(workspace));
    if (static_cast<int64_t>(tb) > room) return GNN_E_ARG;
    int64_t g = (n + kSbBlock - 1) / kSbBlock;
    g = g < 4 * kSbGrid ? g : 4 * kSbGrid;
    hipLaunchKernelGGL(sage_slot_keys_kernel<CENTRE>, dim3(static_cast<unsigned>(g)),
                       dim3(kSbBlock), 0, s, cidx, idx, ldi, M, k, n_prev, w.k0, err_flag);
    GNN_TRY(rocprim::radix_sort_pairs(w.temp, tb, w.k0, w.k1, rocprim::counting_iterator<int32_t>(0),
                                      slot, static_cast<size_t>(n), 0, bits, s));
  }
  const int64_t pb = (n_prev + 1 + kSbBlock - 1) / kSbBlock;
  hipLaunchKernelGGL(sage_slot_ptr_kernel, dim3(static_cast<unsigned>(pb)), dim3(kSbBlock), 0, s,
                     w.k1, n, n_prev, ptr);
  return launch_status();
}

extern "C" int64_t gnn_sage_maps_transpose_workspace_bytes(int64_t M, int64_t k) {
  if (M < 0 || k < 0) return GNN_E_ARG;
  const int64_t n = sb_slots<true>(M, k);
  if (n < 0) return GNN_E_UNSUPPORTED;
  return sb_transpose_carve(nullptr, n).bytes;
}

extern "C" int gnn_sage_maps_transpose(const int64_t* cidx, const int64_t* idx, int64_t ldi,
                                       int64_t M, int64_t k, int64_t n_prev, int64_t* ptr,
                                       int32_t* slot, int32_t* err_flag, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  if (M < 0 || k < 0 || n_prev < 0 || !ptr || !err_flag || !workspace) return GNN_E_ARG;
  if (M > 0 && (!cidx || !slot || (k > 0 && (!idx || ldi < k)))) return GNN_E_ARG;
  const int64_t n = sb_slots<true>(M, k);
  if (n < 0 || n_prev >= 0x7fffffffLL) return GNN_E_UNSUPPORTED;
  return sb_transpose<true>(cidx, idx, ldi, M, k, n_prev, n, ptr, slot, err_flag, workspace,
                            workspace_bytes, stream);
}

// the neighbour map alone (the gcn-mode layer): M k slots, slot e = entry (e / k, e % k)
extern "C" int64_t gnn_sage_maps_transpose_nbr_workspace_bytes(int64_t M, int64_t k) {
  if (M < 0 || k < 0) return GNN_E_ARG;
  const int64_t n = sb_slots<false>(M, k);
  if (n < 0) return GNN_E_UNSUPPORTED;
  return sb_transpose_carve(nullptr, n).bytes;
}

extern "C" int gnn_sage_maps_transpose_nbr(const int64_t* idx, int64_t ldi, int64_t M, int64_t k,
                                           int64_t n_prev, int64_t* ptr, int32_t* slot,
                                           int32_t* err_flag, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
  if (M < 0 || k < 0 || n_prev < 0 || !ptr || !err_flag || !workspace) return GNN_E_ARG;
  if (M > 0 && k > 0 && (!idx || !slot || ldi < k)) return GNN_E_ARG;
  const int64_t n = sb_slots<false>(M, k);
  if (n < 0 || n_prev >= 0x7fffffffLL) return GNN_E_UNSUPPORTED;
  return sb_transpose<false>(nullptr, idx, ldi, M, k, n_prev, n, ptr, slot, err_flag, workspace,
                             workspace_bytes, stream);
}

extern "C" int gnn_sage_scatter_concat_supported(int64_t feat) {
  // F / 4 lanes per row, a power of two of them per wavefront
  return feat >= 4 && feat <= 256 && (feat & (feat - 1)) == 0;
}

template <typename A>
static int dispatch_sage_scatter(const A& a, int64_t feat, hipStream_t s) {
  switch (feat / 4) {
    case 1: return launch_sage_scatter<1>(a, s);
    case 2: return launch_sage_scatter<2>(a, s);
    case 4: return launch_sage_scatter<4>(a, s);
    case 8: return launch_sage_scatter<8>(a, s);
    case 16: return launch_sage_scatter<16>(a, s);
    case 32: return launch_sage_scatter<32>(a, s);
    default: return launch_sage_scatter<64>(a, s);
  }
}

// The body of the four workspace queries. CENTRE: the concat layer (dbuf [M, 2F], the maps of
// gnn_sage_maps_transpose); off: the gcn-mode layer (dbuf [M, F], gnn_sage_maps_transpose_nbr).
// MASK: the MAXPOOL select, whose uint8 winner holds k in [1, 255]; the layout is the MEAN one.
template <bool CENTRE, bool MASK>
static int64_t sb_scatter_bytes(int64_t M, int64_t k, int64_t feat) {
  if (M < 0 || k < 0 || feat < 0) return GNN_E_ARG;
  if (MASK && (k < 1 || k > 255)) return GNN_E_UNSUPPORTED;
  const int64_t n = sb_slots<CENTRE>(M, k);
  if (n < 0 || !gnn_sage_scatter_concat_supported(feat)) return GNN_E_UNSUPPORTED;
  return sb_carve(nullptr, n, feat).bytes;
}

// The body of the five scatter entries (CENTRE, MASK as above; arg / lda are read with MASK
// only). `scale` multiplies every neighbour slot's row of a MEAN form; the select never scales.
template <bool CENTRE, bool MASK>
static int sb_scatter(const float* dbuf, int64_t ldd, const uint8_t* arg, int64_t lda,
                      const int64_t* ptr, const int32_t* slot, int64_t M, int64_t k, int64_t feat,
                      int64_t n_prev, float* dx, int64_t ldx, float scale, void* workspace,
                      int64_t workspace_bytes, void* stream) {
  if (M < 0 || k < 0 || feat < 0 || n_prev < 0) return GNN_E_ARG;
  if (!ptr || !workspace || (n_prev > 0 && !dx) || (M > 0 && (!dbuf || !slot || (MASK && !arg))))
    return GNN_E_ARG;
  const int64_t n = sb_slots<CENTRE>(M, k);
  if (n < 0 || n_prev >= 0x7fffffffLL || !gnn_sage_scatter_concat_supported(feat) ||
      (MASK && (k < 1 || k > 255)))
    return GNN_E_UNSUPPORTED;
  if (ldd < (CENTRE ? 2 * feat : feat) || ldx < feat || (MASK && lda < feat)) return GNN_E_ARG;
  const SbWs w = sb_carve(workspace, n, feat);
  if (workspace_bytes < w.bytes) return GNN_E_ARG;
  if (ldd % 4 || ldx % 4 || !aligned_to(dbuf, 16) || !aligned_to(dx, 16) ||
      (MASK && (lda % 4 || !aligned_to(arg, 4))) || !aligned_to(workspace, 16))
    return GNN_E_ALIGN;
  if (n_prev == 0) return GNN_OK;
  const SbArgs mean{dbuf, ldd, ptr, slot, M, k, n_prev, n, scale, dx, ldx, w.count, w.longs,
                    w.tasks, w.part, w.max_long, w.max_tasks};
  const SbMaskArgs mask{mean, arg, lda};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if constexpr (CENTRE && MASK) return dispatch_sage_scatter(mask, feat, s);
  else if constexpr (CENTRE) return dispatch_sage_scatter(mean, feat, s);
  else if constexpr (MASK) return dispatch_sage_scatter(SbAggMaskArgs{mask}, feat, s);
  else return dispatch_sage_scatter(SbAggArgs{mean}, feat, s);
}

static float sb_inv(int64_t k) { return k > 0 ? 1.0f / static_cast<float>(k) : 0.f; }

extern "C" int64_t gnn_sage_scatter_concat_workspace_bytes(int64_t M, int64_t k, int64_t feat) {
  return sb_scatter_bytes<true, false>(M, k, feat);
}

extern "C" int64_t gnn_sage_scatter_concat_maxpool_workspace_bytes(int64_t M, int64_t k,
                                                                   int64_t feat) {
  return sb_scatter_bytes<true, true>(M, k, feat);
}

extern "C" int64_t gnn_sage_scatter_agg_workspace_bytes(int64_t M, int64_t k, int64_t feat) {
  return sb_scatter_bytes<false, false>(M, k, feat);
}

extern "C" int64_t gnn_sage_scatter_agg_maxpool_workspace_bytes(int64_t M, int64_t k,
                                                                int64_t feat) {
  return sb_scatter_bytes<false, true>(M, k, feat);
}

extern "C" int gnn_sage_scatter_concat_maxpool_f32(const float* dbuf, int64_t ldd,
                                                   const uint8_t* arg, int64_t lda,
                                                   const int64_t* ptr, const int32_t* slot,
                                                   int64_t M, int64_t k, int64_t feat,
                                                   int64_t n_prev, float* dx, int64_t ldx,
                                                   void* workspace, int64_t workspace_bytes,
                                                   void* stream) {
  return sb_scatter<true, true>(dbuf, ldd, arg, lda, ptr, slot, M, k, feat, n_prev, dx, ldx, 1.f,
                                workspace, workspace_bytes, stream);
}

extern "C" int gnn_sage_scatter_concat_f32(const float* dbuf, int64_t ldd, const int64_t* ptr,
                                           const int32_t* slot, int64_t M, int64_t k, int64_t feat,
                                           int64_t n_prev, float* dx, int64_t ldx, void* workspace,
                                           int64_t workspace_bytes, void* stream) {
  return sb_scatter<true, false>(dbuf, ldd, nullptr, 0, ptr, slot, M, k, feat, n_prev, dx, ldx,
                                 sb_inv(k), workspace, workspace_bytes, stream);
}

extern "C" int gnn_sage_scatter_agg_f32(const float* dbuf, int64_t ldd, const int64_t* ptr,
                                        const int32_t* slot, int64_t M, int64_t k, int64_t feat,
                                        int64_t n_prev, float* dx, int64_t ldx, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
  return sb_scatter<false, false>(dbuf, ldd, nullptr, 0, ptr, slot, M, k, feat, n_prev, dx, ldx,
                                  sb_inv(k), workspace, workspace_bytes, stream);
}

// the factor given by the caller (1 for a SUM over the neighbours or a row gather, k = 1)
extern "C" int gnn_sage_scatter_agg_scaled_f32(const float* dbuf, int64_t ldd, const int64_t* ptr,
                                               const int32_t* slot, int64_t M, int64_t k,
                                               int64_t feat, int64_t n_prev, float* dx,
                                               int64_t ldx, float scale, void* workspace,
                                               int64_t workspace_bytes, void* stream) {
  if (k < 1) return k < 0 ? GNN_E_ARG : GNN_E_UNSUPPORTED;
  return sb_scatter<false, false>(dbuf, ldd, nullptr, 0, ptr, slot, M, k, feat, n_prev, dx, ldx,
                                  scale, workspace, workspace_bytes, stream);
}

extern "C" int gnn_sage_scatter_agg_maxpool_f32(const float* dbuf, int64_t ldd, const uint8_t* arg,
                                                int64_t lda, const int64_t* ptr,
                                                const int32_t* slot, int64_t M, int64_t k,
                                                int64_t feat, int64_t n_prev, float* dx,
                                                int64_t ldx, void* workspace,
                                                int64_t workspace_bytes, void* stream) {
  return sb_scatter<false, true>(dbuf, ldd, arg, lda, ptr, slot, M, k, feat, n_prev, dx, ldx, 1.f,
                                 workspace, workspace_bytes, stream);
}
