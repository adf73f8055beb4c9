// relation_product.hip -- boolean sparse x sparse product C = (A . B) > 0, CSR to CSR.
//
// The metapath step of the reference's HAN loader (HAN/utils/data_utils.py:85-89:
// PvsA * PvsA.T, > 0, .toarray()) as structure only: row i of C is the set union of the
// B-rows named by row i of A, written in ascending column order without duplicates -- the
// edge order graph.from_dense(reference_output, "positive") gives.
//
// Two calls (count: rowptr + nnz; fill: col), each recomputing the rows. Nothing is sized by
// the number of partial products sum_i sum_{k in A[i]} deg_B(k): a row is classed by its
// upper bound ub[i] = sum_{k in A[i]} deg_B(k) (int64) and built in place,
//   short  ub <= 64     one wavefront per row: a product per lane, a 64-lane bitonic sort in
//                       registers, neighbours compared for the unique;
//   mid    ub <= 2048   one workgroup per row: an open-addressing table in LDS sized to the
//                       row (>= 2 ub slots, <= 4096), integer CAS inserts, the ids compacted
//                       into a dense LDS array and bitonic-sorted there, then the store;
//   heavy  ub >  2048   a persistent grid, one bitmap of m bits per workgroup in the
//                       workspace: atomicOr of 64-bit words (the words of a lane run merged in
//                       the wave first), popcount, the set bits emitted word by word in
//                       ascending order, and only the word range touched is read and cleared.
// The result is a sorted set, so it is bit-identical from run to run whatever order the
// integer atomics land in. All offsets into rowptr / col are 64-bit.
#include <cstring>  // rocprim's texture_cache_iterator calls host memset

#include <rocprim/rocprim.hpp>

#include "common.hpp"
#include "host.hpp"

namespace gnn {

constexpr int kRpShortMax = 64;     // one product per lane
constexpr int kRpTable = 4096;      // LDS table slots of a mid row (16 KiB; + 8 KiB of ids in fill)
constexpr int kRpMidMax = kRpTable / 2;  // load factor <= 1/2 whatever the row holds
constexpr int kRpBlock = 256;
constexpr int kRpWaves = kRpBlock / kWave;
constexpr int kRpCoopDeg = 32;      // a B-row from this length on is read by the whole wave
constexpr int kRpMidGrid = 4096;    // persistent workgroups over the mid rows
constexpr int kRpHeavyGrid = 256;   // bitmaps (= persistent workgroups) at most ...
constexpr int kRpHeavyGridMin = 16;  // ... and at least
constexpr int64_t kRpBitmapBudget = 256ll << 20;  // bytes of bitmaps aimed at for a large m
constexpr uint32_t kRpEmpty = 0xffffffffu;
constexpr int64_t kRpDimLimit = 0x7fffffffLL;  // n, k, m below 2^31 - 1

struct RpClass {  // rows of one class: lo < ub <= hi
  const int64_t* ub;
  int64_t lo, hi;
  __host__ __device__ bool operator()(int32_t i) const { return ub[i] > lo && ub[i] <= hi; }
};

static int64_t rp_bitmap_words(int64_t m) { return (m + 63) / 64; }

static int rp_heavy_grid(int64_t m) {
  const int64_t bytes = up256(rp_bitmap_words(m) * 8);
  int64_t g = bytes > 0 ? kRpBitmapBudget / bytes : kRpHeavyGrid;
  if (g > kRpHeavyGrid) g = kRpHeavyGrid;
  if (g < kRpHeavyGridMin) g = kRpHeavyGridMin;
  return static_cast<int>(g);
}

static size_t rp_temp_bytes(int64_t n) {
  size_t a = 0, b = 0;
  (void)rocprim::select(nullptr, a, rocprim::counting_iterator<int32_t>(0),
                        static_cast<int32_t*>(nullptr), static_cast<int64_t*>(nullptr),
                        static_cast<size_t>(n > 0 ? n : 1), RpClass{nullptr, 0, 0});
  (void)rocprim::exclusive_scan(nullptr, b, static_cast<int64_t*>(nullptr),
                                static_cast<int64_t*>(nullptr), static_cast<int64_t>(0),
                                static_cast<size_t>(n + 1), rocprim::plus<int64_t>());
  return (a > b ? a : b) + 4096;
}

struct RpWs {
  int64_t* ub;        // [n]
  int64_t* cnt;       // [n + 1]
  int32_t* mid_row;   // [n]
  int32_t* heavy_row;  // [n]
  int64_t* n_class;   // [2] rows in mid_row, heavy_row (device)
  int32_t* err;
  void* temp;
  size_t temp_bytes;
  unsigned long long* bitmap;  // [grid][words]
  int64_t words;      // per bitmap, padded to 256 B
  int grid;
  int64_t bytes;
};

static RpWs rp_carve(void* ws, int64_t n, int64_t m) {
  Carve c{static_cast<char*>(ws)};
  RpWs w{};
  w.ub = c.take<int64_t>(n);
  w.cnt = c.take<int64_t>(n + 1);
  w.mid_row = c.take<int32_t>(n);
  w.heavy_row = c.take<int32_t>(n);
  w.n_class = c.take<int64_t>(2);
  w.err = c.take<int32_t>(1);
  w.temp_bytes = rp_temp_bytes(n);
  w.temp = c.take<char>(static_cast<int64_t>(w.temp_bytes));
  w.words = up256(rp_bitmap_words(m) * 8) / 8;
  w.grid = rp_heavy_grid(m);
  w.bitmap = c.take<unsigned long long>(w.words * w.grid);
  w.bytes = c.used;
  return w;
}

// rowptr[0] == 0, rowptr[rows] == nnz, ascending; every column id inside [0, cols)
__global__ void rp_validate_kernel(const int64_t* __restrict__ rowptr,
                                   const int32_t* __restrict__ col, int64_t rows, int64_t cols,
                                   int64_t nnz, int32_t* __restrict__ err) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  bool bad = false;
  if (i < rows) {
    const int64_t a = rowptr[i], b = rowptr[i + 1];
    bad = a > b || a < 0 || b > nnz;
  }
  if (i == 0) bad = bad || rowptr[0] != 0 || rowptr[rows] != nnz;
  if (i < nnz) {
    const int32_t c = col[i];
    bad = bad || c < 0 || c >= cols;
  }
  if (bad) atomicOr(err, 1);
}

__global__ void rp_bound_kernel(const int64_t* __restrict__ arp, const int32_t* __restrict__ acol,
                                const int64_t* __restrict__ brp, int64_t n,
                                int64_t* __restrict__ ub, int64_t* __restrict__ cnt) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i == 0) cnt[n] = 0;
  if (i >= n) return;
  int64_t s = 0;
  for (int64_t e = arp[i]; e < arp[i + 1]; ++e) {
    const int32_t r = acol[e];
    s += brp[r + 1] - brp[r];
  }
  ub[i] = s;
  if (s == 0) cnt[i] = 0;  // no class visits an empty row
}

// ---------------------------------------------------------------------------- short rows
template <bool FILL>
__global__ __launch_bounds__(kRpBlock) void rp_short_kernel(
    const int64_t* __restrict__ arp, const int32_t* __restrict__ acol,
    const int64_t* __restrict__ brp, const int32_t* __restrict__ bcol, int64_t n,
    const int64_t* __restrict__ ub, int64_t* __restrict__ cnt,
    const int64_t* __restrict__ crp, int32_t* __restrict__ ccol, int64_t nnz_c) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kRpWaves + (threadIdx.x >> 6);
  if (i >= n) return;
  const int64_t u = ub[i];
  if (u <= 0 || u > kRpShortMax) return;
  const int64_t a_beg = arp[i], a_end = arp[i + 1];
  int32_t v = 0x7fffffff;  // no column id reaches it (m < 2^31 - 1)
  int base = 0;            // products placed so far: lane base + t takes product t of a B-row
  for (int64_t c0 = a_beg; c0 < a_end; c0 += kWave) {
    const int64_t e = c0 + lane;
    int64_t bb = 0;
    int bd = 0;
    if (e < a_end) {
      const int32_t r = acol[e];
      bb = brp[r];
      bd = static_cast<int>(brp[r + 1] - bb);  // <= ub <= 64
    }
    uint64_t nz = __ballot(bd > 0);
    while (nz) {
      const int j = __ffsll(static_cast<unsigned long long>(nz)) - 1;
      nz &= nz - 1;
      const int64_t b0 = __shfl(bb, j, kWave);
      const int d0 = __shfl(bd, j, kWave);
      const int t = lane - base;
      if (t >= 0 && t < d0) v = bcol[b0 + t];
      base += d0;
    }
  }
  // bitonic sort of the 64 lanes, ascending
  for (int k = 2; k <= kWave; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int32_t o = __shfl_xor(v, j, kWave);
      const bool up = (lane & k) == 0 || k == kWave;
      const bool low = (lane & j) == 0;
      v = (low == up) ? min(v, o) : max(v, o);
    }
  }
  const int32_t prev = __shfl_up(v, 1, kWave);
  const bool keep = v != 0x7fffffff && (lane == 0 || prev != v);
  const uint64_t km = __ballot(keep);
  if (!FILL) {
    if (lane == 0) cnt[i] = __popcll(km);
  } else {
    const int64_t dst = crp[i] + __popcll(km & ((1ull << lane) - 1));
    if (keep && dst < crp[i + 1] && dst < nnz_c) ccol[dst] = v;
  }
}

// ------------------------------------------------------- the products of one row, per wave
// Wave `wave` of `nwaves` takes chunks of 64 entries of A's row: a lane reads one entry's B-row
// bounds; B-rows of kRpCoopDeg ids or more are then read by the whole wave, 64 ids a step
// (sink.coop, every lane calls it), the others by their own lane (sink.one).
template <class Sink>
__device__ __forceinline__ void rp_row_products(const int32_t* __restrict__ acol,
                                                const int64_t* __restrict__ brp,
                                                const int32_t* __restrict__ bcol, int64_t a_beg,
                                                int64_t a_end, int wave, int nwaves, int lane,
                                                Sink& sink) {
  for (int64_t c0 = a_beg + static_cast<int64_t>(wave) * kWave; c0 < a_end;
       c0 += static_cast<int64_t>(nwaves) * kWave) {
    const int64_t e = c0 + lane;
    int64_t bb = 0, bd = 0;
    if (e < a_end) {
      const int32_t r = acol[e];
      bb = brp[r];
      bd = brp[r + 1] - bb;
    }
    uint64_t lm = __ballot(bd >= kRpCoopDeg);
    while (lm) {
      const int j = __ffsll(static_cast<unsigned long long>(lm)) - 1;
      lm &= lm - 1;
      const int64_t b0 = __shfl(bb, j, kWave);
      const int64_t d0 = __shfl(bd, j, kWave);
      for (int64_t t0 = 0; t0 < d0; t0 += kWave) {
        const int64_t t = t0 + lane;
        const bool valid = t < d0;
        sink.coop(valid ? bcol[b0 + t] : 0, valid, lane);
      }
    }
    if (bd < kRpCoopDeg)
      for (int64_t t = 0; t < bd; ++t) sink.one(bcol[bb + t]);
  }
}

// ------------------------------------------------------------------------------ mid rows
struct RpTableSink {
  uint32_t* tab;
  uint32_t mask;
  int shift;
  int added;
  __device__ __forceinline__ void one(int32_t c) {
    const uint32_t v = static_cast<uint32_t>(c);
    uint32_t s = (v * 0x9e3779b1u) >> shift;  // multiplicative: ids congruent mod 2^k spread
    for (;;) {  // ends: the row holds <= ub <= slots / 2 distinct ids
      const uint32_t old = atomicCAS(&tab[s], kRpEmpty, v);
      if (old == kRpEmpty) {
        ++added;
        return;
      }
      if (old == v) return;
      s = (s + 1) & mask;
    }
  }
  __device__ __forceinline__ void coop(int32_t c, bool valid, int) {
    if (valid) one(c);
  }
};

template <bool FILL>
__global__ __launch_bounds__(kRpBlock) void rp_mid_kernel(
    const int64_t* __restrict__ arp, const int32_t* __restrict__ acol,
    const int64_t* __restrict__ brp, const int32_t* __restrict__ bcol,
    const int32_t* __restrict__ rows, const int64_t* __restrict__ n_rows,
    const int64_t* __restrict__ ub, int64_t* __restrict__ cnt,
    const int64_t* __restrict__ crp, int32_t* __restrict__ ccol, int64_t nnz_c) {
  __shared__ uint32_t tab[kRpTable];
  __shared__ uint32_t dense[FILL ? kRpMidMax : 1];  // the row's ids, compacted, for the sort
  __shared__ int s_wave[kRpWaves];
  __shared__ int total;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int64_t nr = *n_rows;
  for (int64_t q = blockIdx.x; q < nr; q += gridDim.x) {
    const int64_t i = rows[q];
    const int64_t u = ub[i];  // kRpShortMax < u <= kRpMidMax
    int slots = 2 * kRpShortMax;
    int shift = 32 - 7;
    while (slots < 2 * u && slots < kRpTable) {
      slots <<= 1;
      --shift;
    }
    for (int s = tid; s < slots; s += kRpBlock) tab[s] = kRpEmpty;
    if (tid == 0) total = 0;
    __syncthreads();
    RpTableSink sink{tab, static_cast<uint32_t>(slots - 1), shift, 0};
    rp_row_products(acol, brp, bcol, arp[i], arp[i + 1], wave, kRpWaves, lane, sink);
    if (!FILL) {
      if (sink.added) atomicAdd(&total, sink.added);
      __syncthreads();
      if (tid == 0) cnt[i] = total;
      __syncthreads();  // total and tab are reused by the next row
      continue;
    }
    __syncthreads();
    // the ids leave the table for a dense array (in any order), padded with empty marks to a
    // power of two: the bitonic sort then runs over the ids, not over the table's empty slots
    int c = 0;
    for (int s = tid; s < slots; s += kRpBlock) c += tab[s] != kRpEmpty;
    int incl = c;  // inclusive scan over the wave
    for (int d = 1; d < kWave; d <<= 1) {
      const int o = __shfl_up(incl, d, kWave);
      if (lane >= d) incl += o;
    }
    if (lane == kWave - 1) s_wave[wave] = incl;
    __syncthreads();
    int o = incl - c, count = 0;
    for (int x = 0; x < kRpWaves; ++x) {
      if (x < wave) o += s_wave[x];
      count += s_wave[x];
    }
    for (int s = tid; s < slots; s += kRpBlock) {
      const uint32_t v = tab[s];
      if (v != kRpEmpty) dense[o++] = v;  // count <= ub <= kRpMidMax
    }
    int sorted = 2;
    while (sorted < count) sorted <<= 1;
    for (int s = count + tid; s < sorted; s += kRpBlock) dense[s] = kRpEmpty;
    __syncthreads();
    for (int k = 2; k <= sorted; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < sorted / 2; t += kRpBlock) {
          const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int hi = lo | j;
          const uint32_t x = dense[lo], y = dense[hi];
          const bool up = (lo & k) == 0;
          if ((x > y) == up) {
            dense[lo] = y;
            dense[hi] = x;
          }
        }
        __syncthreads();
      }
    }
    const int64_t dst = crp[i], end = crp[i + 1];
    for (int s = tid; s < count; s += kRpBlock)
      if (dst + s < end && dst + s < nnz_c) ccol[dst + s] = static_cast<int32_t>(dense[s]);
    __syncthreads();  // tab, dense and s_wave are reused by the next row
  }
}

// ---------------------------------------------------------------------------- heavy rows
struct RpBitmapSink {
  unsigned long long* bm;
  int64_t wmin, wmax;
  __device__ __forceinline__ void set(int64_t w, unsigned long long bits) {
    atomicOr(&bm[w], bits);
    wmin = w < wmin ? w : wmin;
    wmax = w > wmax ? w : wmax;
  }
  __device__ __forceinline__ void one(int32_t c) { set(c >> 6, 1ull << (c & 63)); }
  // 64 ids of one B-row: the bits of a run of lanes that share a word are merged first, and
  // the run's first lane sets them (a B-row in ascending order is one atomic per word)
  __device__ __forceinline__ void coop(int32_t c, bool valid, int lane) {
    const int w = valid ? (c >> 6) : -1;
    unsigned long long bits = valid ? 1ull << (c & 63) : 0ull;
    for (int d = 1; d < kWave; d <<= 1) {
      const int ow = __shfl_down(w, d, kWave);
      const unsigned long long ob = __shfl_down(bits, d, kWave);
      if (lane + d < kWave && ow == w) bits |= ob;
    }
    const int pw = __shfl_up(w, 1, kWave);
    if (valid && (lane == 0 || pw != w)) set(w, bits);
  }
};

template <bool FILL>
__global__ __launch_bounds__(kRpBlock) void rp_heavy_kernel(
    const int64_t* __restrict__ arp, const int32_t* __restrict__ acol,
    const int64_t* __restrict__ brp, const int32_t* __restrict__ bcol,
    const int32_t* __restrict__ rows, const int64_t* __restrict__ n_rows,
    unsigned long long* __restrict__ bitmaps, int64_t words, int64_t* __restrict__ cnt,
    const int64_t* __restrict__ crp, int32_t* __restrict__ ccol, int64_t nnz_c) {
  __shared__ int s_min, s_max;  // word indices: < 2^25
  __shared__ long long s_run;
  __shared__ int s_wave[kRpWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  unsigned long long* bm = bitmaps + static_cast<int64_t>(blockIdx.x) * words;  // all zero
  const int64_t nr = *n_rows;
  for (int64_t q = blockIdx.x; q < nr; q += gridDim.x) {
    const int64_t i = rows[q];
    if (tid == 0) {
      s_min = static_cast<int>(words);
      s_max = -1;
      s_run = 0;
    }
    __syncthreads();
    RpBitmapSink sink{bm, words, -1};
    rp_row_products(acol, brp, bcol, arp[i], arp[i + 1], wave, kRpWaves, lane, sink);
    if (sink.wmax >= 0) {
      atomicMin(&s_min, static_cast<int>(sink.wmin));
      atomicMax(&s_max, static_cast<int>(sink.wmax));
    }
    // the atomics have reached L2 before another wave of the workgroup reads the words there
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int64_t w_lo = s_min, w_hi = s_max;
    const int64_t dst = FILL ? crp[i] : 0, end = FILL ? crp[i + 1] : 0;
    // the touched word range, 256 words a step: read, clear, count, emit
    for (int64_t w0 = w_lo; w0 <= w_hi; w0 += kRpBlock) {
      const int64_t w = w0 + tid;
      unsigned long long bits = 0;
      if (w <= w_hi) {
        bits = __hip_atomic_load(&bm[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (bits) __hip_atomic_store(&bm[w], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      const int c = __popcll(bits);
      int incl = c;  // inclusive scan over the wave
      for (int d = 1; d < kWave; d <<= 1) {
        const int o = __shfl_up(incl, d, kWave);
        if (lane >= d) incl += o;
      }
      if (lane == kWave - 1) s_wave[wave] = incl;
      __syncthreads();
      int before = 0, step = 0;
      for (int x = 0; x < kRpWaves; ++x) {
        if (x < wave) before += s_wave[x];
        step += s_wave[x];
      }
      const int64_t run = s_run;
      if (FILL) {
        int64_t o = dst + run + before + incl - c;
        const int64_t id0 = w * 64;
        while (bits) {
          const int b = __ffsll(bits) - 1;
          bits &= bits - 1;
          if (o < end && o < nnz_c) ccol[o] = static_cast<int32_t>(id0 + b);
          ++o;
        }
      }
      __syncthreads();  // every thread has read s_run and s_wave
      if (tid == 0) s_run = run + step;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clearing stores, before the next row
    __syncthreads();
    if (!FILL && tid == 0) cnt[i] = s_run;
    __syncthreads();  // s_min / s_max / s_run are reset by the next row
  }
}

static int rp_check_dims(int64_t n, int64_t k, int64_t m, int64_t nnz_a, int64_t nnz_b) {
  if (n < 0 || k < 0 || m < 0 || nnz_a < 0 || nnz_b < 0) return GNN_E_ARG;
  if (n >= kRpDimLimit || k >= kRpDimLimit || m >= kRpDimLimit) return GNN_E_UNSUPPORTED;
  return GNN_OK;
}

template <bool FILL>
static void rp_launch_rows(const int64_t* arp, const int32_t* acol, const int64_t* brp,
                           const int32_t* bcol, int64_t n, const RpWs& w, const int64_t* crp,
                           int32_t* ccol, int64_t nnz_c, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(rp_short_kernel<FILL>, dim3(blocks(n, kRpWaves)), dim3(kRpBlock), 0, s, arp,
                     acol, brp, bcol, n, w.ub, w.cnt, crp, ccol, nnz_c);
  const int64_t mid_grid = n < kRpMidGrid ? n : kRpMidGrid;
  hipLaunchKernelGGL(rp_mid_kernel<FILL>, dim3(static_cast<unsigned>(mid_grid)), dim3(kRpBlock), 0,
                     s, arp, acol, brp, bcol, w.mid_row, w.n_class, w.ub, w.cnt, crp, ccol, nnz_c);
  const int64_t heavy_grid = n < w.grid ? n : w.grid;
  hipLaunchKernelGGL(rp_heavy_kernel<FILL>, dim3(static_cast<unsigned>(heavy_grid)),
                     dim3(kRpBlock), 0, s, arp, acol, brp, bcol, w.heavy_row, w.n_class + 1,
                     w.bitmap, w.words, w.cnt, crp, ccol, nnz_c);
}

}  // namespace gnn

using namespace gnn;

extern "C" int64_t gnn_relation_product_workspace_bytes(int64_t n, int64_t k, int64_t m,
                                                        int64_t nnz_a, int64_t nnz_b) {
  const int rc = rp_check_dims(n, k, m, nnz_a, nnz_b);
  if (rc != GNN_OK) return rc;
  // the terms: O(n) row arrays and rocPRIM's temporaries, and a fixed number of m-bit bitmaps
  return rp_carve(nullptr, n, m).bytes + 256;
}

extern "C" int gnn_relation_product_class_limits(int64_t* short_max, int64_t* mid_max) {
  if (!short_max || !mid_max) return GNN_E_ARG;
  *short_max = kRpShortMax;
  *mid_max = kRpMidMax;
  return GNN_OK;
}

extern "C" int gnn_relation_product_count(const int64_t* a_rowptr, const int32_t* a_col,
                                          int64_t nnz_a, const int64_t* b_rowptr,
                                          const int32_t* b_col, int64_t nnz_b, int64_t n,
                                          int64_t k, int64_t m, int64_t* c_rowptr,
                                          int64_t* nnz_out, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
  const int rc = rp_check_dims(n, k, m, nnz_a, nnz_b);
  if (rc != GNN_OK) return rc;
  if (!a_rowptr || !b_rowptr || !c_rowptr || !nnz_out || !workspace || (nnz_a > 0 && !a_col) ||
      (nnz_b > 0 && !b_col))
    return GNN_E_ARG;
  RpWs w = rp_carve(workspace, n, m);
  if (workspace_bytes < w.bytes + 256) return GNN_E_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  GNN_TRY(hipMemsetAsync(w.err, 0, sizeof(int32_t), s));
  GNN_TRY(hipMemsetAsync(w.n_class, 0, 2 * sizeof(int64_t), s));
  GNN_TRY(hipMemsetAsync(w.bitmap, 0, static_cast<size_t>(w.words) * 8 * w.grid, s));
  const int64_t va = (n > nnz_a ? n : nnz_a) + 1, vb = (k > nnz_b ? k : nnz_b) + 1;
  hipLaunchKernelGGL(rp_validate_kernel, dim3(blocks(va, 256)), dim3(256), 0, s, a_rowptr, a_col,
                     n, k, nnz_a, w.err);
  hipLaunchKernelGGL(rp_validate_kernel, dim3(blocks(vb, 256)), dim3(256), 0, s, b_rowptr, b_col,
                     k, m, nnz_b, w.err);
  int32_t herr = 0;
  GNN_TRY(sync_read(w.err, &herr, 1, s));
  if (herr) return GNN_E_ARG;  // an id outside its range (or a broken rowptr): nothing follows it
  hipLaunchKernelGGL(rp_bound_kernel, dim3(blocks(n + 1, 256)), dim3(256), 0, s, a_rowptr, a_col,
                     b_rowptr, n, w.ub, w.cnt);
  if (n > 0) {
    size_t tb = w.temp_bytes;
    GNN_TRY(rocprim::select(w.temp, tb, rocprim::counting_iterator<int32_t>(0), w.mid_row,
                            w.n_class, static_cast<size_t>(n),
                            RpClass{w.ub, kRpShortMax, kRpMidMax}, s));
    tb = w.temp_bytes;
    GNN_TRY(rocprim::select(w.temp, tb, rocprim::counting_iterator<int32_t>(0), w.heavy_row,
                            w.n_class + 1, static_cast<size_t>(n),
                            RpClass{w.ub, kRpMidMax, INT64_MAX}, s));
  }
  rp_launch_rows<false>(a_rowptr, a_col, b_rowptr, b_col, n, w, nullptr, nullptr, 0, s);
  size_t tb = w.temp_bytes;
  GNN_TRY(rocprim::exclusive_scan(w.temp, tb, w.cnt, c_rowptr, static_cast<int64_t>(0),
                                  static_cast<size_t>(n + 1), rocprim::plus<int64_t>(), s));
  int64_t nnz = 0;
  GNN_TRY(sync_read(c_rowptr + n, &nnz, 1, s));
  *nnz_out = nnz;
  return launch_status();
}

extern "C" int gnn_relation_product_fill(const int64_t* a_rowptr, const int32_t* a_col,
                                         int64_t nnz_a, const int64_t* b_rowptr,
                                         const int32_t* b_col, int64_t nnz_b, int64_t n, int64_t k,
                                         int64_t m, const int64_t* c_rowptr, int32_t* c_col,
                                         int64_t nnz_c, void* workspace, int64_t workspace_bytes,
                                         void* stream) {
  const int rc = rp_check_dims(n, k, m, nnz_a, nnz_b);
  if (rc != GNN_OK) return rc;
  if (!a_rowptr || !b_rowptr || !c_rowptr || !workspace || nnz_c < 0 || (nnz_c > 0 && !c_col) ||
      (nnz_a > 0 && !a_col) || (nnz_b > 0 && !b_col))
    return GNN_E_ARG;
  RpWs w = rp_carve(workspace, n, m);
  if (workspace_bytes < w.bytes + 256) return GNN_E_ARG;
  if (nnz_c == 0) return GNN_OK;
  rp_launch_rows<true>(a_rowptr, a_col, b_rowptr, b_col, n, w, c_rowptr, c_col, nnz_c,
                       static_cast<hipStream_t>(stream));
  return launch_status();
}
