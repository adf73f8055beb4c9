// unsup.hip -- the two producers of an unsupervised GraphSAGE batch on gfx950: a node's
// positive contexts (gnn_sample_contexts, get_context_nodes, GraphSAGE/data_utils.py:50-58) and
// its negatives (gnn_sample_negatives, get_negative_nodes, data_utils.py:61-70). Both follow the
// sampler's design (sample_kernels.hpp): the counter RNG keyed by (seed, position, draw), a
// group of lanes per node, error bits instead of exceptions, a nullable device row count.
//
// Contexts. Lane l of a node's group owns output column l:
//   deg >  window : col[rowptr[v] + l] -- the first `window` entries of the CSR row. The
//                   reference takes the first `window` of list(set), an arbitrary but fixed
//                   subset; here it is CSR order (ascending ids after symmetric_adjacency);
//   deg <= window : col[rowptr[v] + uniform_below(seed, i, l, deg)] -- random.choices, with
//                   replacement (deg == window too: the reference's test is a strict >);
//   deg == 0      : a row of -1, kSampleErrEmpty; a node id outside the graph: kSampleErrRange.
//
// Negatives. Row i is the first need = window * K ACCEPTED candidates of the stream
//   c_t = uniform_below(seed, i, t, n_nodes),  t = 0, 1, ...
// where c_t is accepted iff it equals no context of row i and no earlier accepted candidate of
// row i (the reference's `neg not in contexts and neg not in negatives`; like the reference the
// centre node itself is not excluded). A group of G lanes evaluates G stream positions per
// round: lane s holds c_{t0 + s}, tests it against the row's contexts and the accepted list
// (both in LDS) and against the earlier lanes of the round (a candidate equal to an earlier
// lane's is rejected whatever became of that lane: if the earlier one was accepted it is a
// repeat, and if it was rejected for a context / accepted id / the cut, so is this one). One
// ballot and a prefix popcount hand the survivors their slots in stream order; slots from
// `need` on are dropped, exactly where the sequential loop stops. The result therefore does
// not depend on G.
//
// The reference loops forever when fewer than `need` ids are allowed. Here a row whose
// distinct in-range contexts d leave n_nodes - d < need ids is refused up front (a row of -1,
// kNegErrInfeasible), and a feasible row's stream is cut at
//   T_max = 64 * need + 4096
// positions (kNegErrInternal if ever reached, the policy of the frontier scan's bounded
// look-back). Derivation: with a >= need allowed ids among n = a + d, the row is short after T
// draws only if at least a - need + 1 allowed ids were never drawn; the worst case is
// a = need = m (every allowed id must appear), where the union bound over the m ids gives
//   P <= m (1 - 1/(m + d))^T <= m exp(-T / (m + d)).
// For a > need the row needs only `need` of more ids, each as likely: P is smaller. With
// d <= window <= 64 and m <= 1024: T_max / (m + d) >= (64 m + 4096) / (m + 64) = 64, so
// P <= 1024 e^-64 = 2^(10 - 92.3) < 2^-82 < 2^-64.
#include "sample_kernels.hpp"

using namespace gnn;

namespace gnn {

constexpr int32_t kNegErrInfeasible = 32;  // (1..16 are the neighbour sampler's and the batch's)
constexpr int32_t kNegErrInternal = 64;
constexpr int kMaxWindow = 64;
constexpr int kMaxNeed = 1024;

// *err |= bit, skipping the atomic once the bit is seen set: a dataset-scale call over a graph
// where many nodes fail (4.4M of the cfg4 R-MAT's 10M nodes have no neighbour) otherwise
// serialises millions of atomics on one word (12.9 ms instead of the gather's own time)
__device__ __forceinline__ void raise_bit(int32_t* err, int32_t bit) {
  if ((__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) == 0)
    atomicOr(err, bit);
}

template <int LPN>
__global__ __launch_bounds__(256) void contexts_kernel(const int64_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ col,
                                                       int64_t n_graph,
                                                       const int64_t* __restrict__ nodes, int64_t n,
                                                       const int64_t* n_dev, int window,
                                                       uint64_t seed, int64_t* __restrict__ out,
                                                       int32_t* __restrict__ err) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t i = t / LPN;
  const int sub = static_cast<int>(t & (LPN - 1));
  if (i >= live_rows(n, n_dev) || sub >= window) return;
  const int64_t v = nodes[i];
  int64_t* o = out + i * window + sub;
  if (v < 0 || v >= n_graph) {
    if (sub == 0) raise_bit(err, kSampleErrRange);
    *o = -1;
    return;
  }
  const int64_t b = rowptr[v];
  const int64_t deg = rowptr[v + 1] - b;
  if (deg == 0) {
    if (sub == 0) raise_bit(err, kSampleErrEmpty);
    *o = -1;
    return;
  }
  const int64_t pick = deg > window ? sub : uniform_below(seed, i, sub, deg);
  *o = col[b + pick];
}

// does lane `src` hold the same id? The low word alone decides while every id fits 31 bits
__device__ __forceinline__ bool same_as_lane(int64_t mine, int src, bool wide) {
  const uint32_t lo = static_cast<uint32_t>(mine), hi = static_cast<uint32_t>(mine >> 32);
  bool eq = __shfl(lo, src, kWave) == lo;
  if (wide) eq = eq && __shfl(hi, src, kWave) == hi;  // wave-uniform branch
  return eq;
}

// G lanes per row, kWave / G rows per wave, 4 waves per workgroup. LDS: per row `window`
// contexts then `need` accepted ids. Every loop that holds a cross-lane operation runs a
// wave-uniform number of times (rows that are done idle through it).
template <int G>
__global__ __launch_bounds__(256) void negatives_kernel(const int64_t* __restrict__ contexts,
                                                        int64_t n, const int64_t* n_dev,
                                                        int window, int need, int64_t n_nodes,
                                                        uint64_t seed, int64_t* __restrict__ out,
                                                        int32_t* __restrict__ err) {
  extern __shared__ int64_t lds[];
  constexpr int GPW = kWave / G;
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane & (G - 1);
  const int gbase = lane & ~(G - 1);
  const uint64_t gmask = (G == 64 ? ~0ull : ((1ull << G) - 1)) << gbase;
  const uint64_t below = gmask & ((1ull << lane) - 1);  // this row's lanes before this one
  const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  const int64_t live = live_rows(n, n_dev);
  if (wave * GPW >= live) return;  // wave-uniform
  const int64_t i = wave * GPW + lane / G;
  const bool act = i < live;
  int64_t* ctx = lds + static_cast<int64_t>(threadIdx.x / G) * (window + need);
  int64_t* acc = ctx + window;
  const bool wide = n_nodes > 0x7fffffffll;  // (an idle lane's -1 - lane has the top bit set)

  // the row's contexts (G >= window), and d = how many distinct ids of [0, n_nodes) they hold
  const bool has = act && sub < window;
  const int64_t c = has ? contexts[i * window + sub] : -1;
  if (has) ctx[sub] = c;
  bool first = has && c >= 0 && c < n_nodes;
  for (int jj = 0; jj < window; ++jj)
    if (same_as_lane(c, gbase + jj, true) && jj < sub) first = false;
  const int d = __popcll(__ballot(first) & gmask);
  const bool feasible = act && n_nodes - d >= need;
  if (act && !feasible && sub == 0) raise_bit(err, kNegErrInfeasible);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  const int64_t t_max = 64ll * need + 4096;
  int cnt = 0;
  int64_t t0 = 0;
  while (__any(feasible && cnt < need && t0 < t_max)) {
    const bool run = feasible && cnt < need && t0 < t_max;
    const int64_t t = t0 + sub;
    int64_t cand = -1 - lane;  // idle lanes: distinct ids no candidate equals
    bool ok = run && t < t_max;
    if (ok) {
      cand = uniform_below(seed, i, t, n_nodes);
      for (int j = 0; j < window; ++j) ok = ok && ctx[j] != cand;
      for (int j = 0; j < cnt; ++j) ok = ok && acc[j] != cand;
    }
    for (int jj = 0; jj < G - 1; ++jj)  // first occurrence in the round wins
      if (same_as_lane(cand, gbase + jj, wide) && jj < sub) ok = false;
    const uint64_t won = __ballot(ok) & gmask;
    const int slot = cnt + __popcll(won & below);
    if (ok && slot < need) {
      acc[slot] = cand;
      out[i * need + slot] = cand;
    }
    if (run) {
      cnt = min(need, cnt + __popcll(won));
      t0 += G;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  if (!act) return;
  if (feasible && cnt < need && sub == 0) raise_bit(err, kNegErrInternal);
  for (int j = (feasible ? cnt : 0) + sub; j < need; j += G) out[i * need + j] = -1;
}

template <int G>
void launch_negatives(const int64_t* contexts, int64_t n, const int64_t* n_dev, int window,
                      int need, int64_t n_nodes, uint64_t seed, int64_t* out, int32_t* err,
                      hipStream_t s) {
  constexpr int rows_per_block = 4 * (kWave / G);
  const dim3 grid(static_cast<unsigned>((n + rows_per_block - 1) / rows_per_block));
  const size_t lds = static_cast<size_t>(rows_per_block) * (window + need) * sizeof(int64_t);
  hipLaunchKernelGGL(negatives_kernel<G>, grid, dim3(256), lds, s, contexts, n, n_dev, window,
                     need, n_nodes, seed, out, err);
}

}  // namespace gnn

extern "C" int gnn_sample_contexts(const int64_t* rowptr, const int32_t* col, int64_t n_graph,
                                   const int64_t* nodes, int64_t n, const int64_t* n_dev,
                                   int64_t window, uint64_t seed, int64_t* out, int32_t* err_flag,
                                   void* stream) {
  if (n < 0 || n_graph < 0) return GNN_E_ARG;
  if (window < 1 || window > kMaxWindow) return GNN_E_UNSUPPORTED;
  if (!rowptr || !col || !nodes || !out || !err_flag) return GNN_E_ARG;
  if (n == 0) return GNN_OK;
  const int lpn = window <= 16 ? 16 : window <= 32 ? 32 : 64;
  const int64_t blocks = (n * lpn + 255) / 256;
  if (blocks > 0x7fffffffLL) return GNN_E_UNSUPPORTED;
  const dim3 g(static_cast<unsigned>(blocks)), t(256);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int w = static_cast<int>(window);
  if (lpn == 16)
    hipLaunchKernelGGL(contexts_kernel<16>, g, t, 0, s, rowptr, col, n_graph, nodes, n, n_dev, w,
                       seed, out, err_flag);
  else if (lpn == 32)
    hipLaunchKernelGGL(contexts_kernel<32>, g, t, 0, s, rowptr, col, n_graph, nodes, n, n_dev, w,
                       seed, out, err_flag);
  else
    hipLaunchKernelGGL(contexts_kernel<64>, g, t, 0, s, rowptr, col, n_graph, nodes, n, n_dev, w,
                       seed, out, err_flag);
  return launch_status();
}

extern "C" int gnn_sample_negatives(const int64_t* contexts, int64_t n, const int64_t* n_dev,
                                    int64_t window, int64_t need, int64_t n_nodes, uint64_t seed,
                                    int64_t* out, int32_t* err_flag, void* stream) {
  if (n < 0 || n_nodes < 0) return GNN_E_ARG;
  if (window < 1 || window > kMaxWindow || need < 1 || need > kMaxNeed) return GNN_E_UNSUPPORTED;
  if (!contexts || !out || !err_flag) return GNN_E_ARG;
  if (n == 0) return GNN_OK;
  // G >= min(need, 64) lanes per row, and G >= window: the group also holds the contexts
  const int64_t width = need > window ? need : window;
  const int G = width <= 16 ? 16 : width <= 32 ? 32 : 64;
  if ((n + 4 * (kWave / G) - 1) / (4 * (kWave / G)) > 0x7fffffffLL) return GNN_E_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int w = static_cast<int>(window), m = static_cast<int>(need);
  if (G == 16) launch_negatives<16>(contexts, n, n_dev, w, m, n_nodes, seed, out, err_flag, s);
  else if (G == 32) launch_negatives<32>(contexts, n, n_dev, w, m, n_nodes, seed, out, err_flag, s);
  else launch_negatives<64>(contexts, n, n_dev, w, m, n_nodes, seed, out, err_flag, s);
  return launch_status();
}
