// induced_subgraph.hip -- induced subgraph C = A[idx][:, idx], CSR to CSR, values carried.
//
// The mini-batch slice of the reference's HAN loader (HAN/utils/data_utils.py:98-101,
// collect_f.__call__: HG_adj[idx][:, idx] on a dense N x N tensor) without the dense array:
// C[r, p] = A[idx[r], idx[p]], row r of C in ascending position order -- the edge order
// graph.from_dense(dense(A)[idx][:, idx], ...) gives.
//
// Three calls per batch, none of which synchronises the stream:
//   map    id -> positions of this batch: head[v] = one position that holds id v (or -1),
//          next[p] = another position with idx[p]'s id (or -1), clen[head[v]] = how many
//          positions hold v. Built with integer atomic exchanges, so the order inside a chain
//          is whatever order they land in; nothing below depends on it.
//   count  a wavefront per selected row reads 64 entries of A's row per step, looks each
//          column up in head and adds its chain length; one rocprim::exclusive_scan gives
//          c_rowptr.
//   fill   rows are classed by their KEPT count c = c_rowptr[r+1] - c_rowptr[r]:
//            short  c <= 64    one wavefront: the kept (position, ordinal) keys compacted by a
//                              wave prefix sum, a 64-lane bitonic sort of the 64-bit keys in
//                              registers, the value fetched through the ordinal;
//            mid    c <= 2048  one workgroup per row on a persistent grid: compaction and
//                              bitonic sort of the keys in LDS;
//            heavy  c >  2048  rank by bitmap: atomicOr of the position bits into a bitmap of
//                              b bits (in LDS while b <= 131072, else one bitmap per workgroup in
//                              the workspace), a word-prefix popcount over the touched words,
//                              each kept entry stored at c_rowptr[r] + rank(position).
//          The short kernel visits every row and queues the mid and heavy rows (integer
//          atomics: the queue order varies, the rows' outputs do not).
// The result is a sorted sequence, so it is bit-identical from run to run whatever order the
// integer atomics land in. All offsets into rowptr / col / val are 64-bit.
#include <cstring>  // rocprim's texture_cache_iterator calls host memset

#include <rocprim/rocprim.hpp>

#include "common.hpp"
#include "host.hpp"

namespace gnn {

constexpr int kIsShortMax = 64;        // one key per lane
constexpr int kIsMidMax = 2048;        // keys of a mid row in LDS (16 KiB)
constexpr int64_t kIsLdsBits = 131072;  // bitmap (16 KiB) + word prefix (8 KiB) in LDS
constexpr int kIsLdsWords = static_cast<int>(kIsLdsBits / 64);
constexpr int kIsBlock = 256;
constexpr int kIsWaves = kIsBlock / kWave;
constexpr int kIsMidGrid = 2048;       // persistent workgroups over the mid rows
constexpr int kIsHeavyGridLds = 1024;  // ... over the heavy rows, bitmap in LDS
constexpr int kIsHeavyGridWs = 64;     // ... bitmaps in the workspace (a fixed number of them)
constexpr int64_t kIsDimLimit = 0x7fffffffLL;  // n, b below 2^31 - 1
constexpr int kIsBadIdx = 1, kIsBadGraph = 2, kIsRepeat = 4;  // status bits 0, 1, 2
constexpr unsigned long long kIsNoKey = ~0ull;

static size_t is_temp_bytes(int64_t b) {
  size_t need = 0;
  (void)rocprim::exclusive_scan(nullptr, need, static_cast<int64_t*>(nullptr),
                                static_cast<int64_t*>(nullptr), static_cast<int64_t>(0),
                                static_cast<size_t>(b + 1), rocprim::plus<int64_t>());
  // rocPRIM's need is a few bytes per scanned block; the floor keeps the query non-decreasing in b
  const size_t floor_bytes = static_cast<size_t>(65536 + b / 4);
  return need > floor_bytes ? need : floor_bytes;
}

struct IsWs {
  // map part: read-only after gnn_induced_subgraph_map
  int32_t* head;  // [n]
  int32_t* next;  // [b]
  int32_t* clen;  // [b], valid at head positions
  // scratch part: any count or fill may overwrite it
  int64_t* cnt;        // [b + 1]
  int32_t* mid_row;    // [b]
  int32_t* heavy_row;  // [b]
  int32_t* n_class;    // [2] rows queued in mid_row, heavy_row
  void* temp;
  size_t temp_bytes;
  unsigned long long* bitmap;  // [kIsHeavyGridWs][words], only above kIsLdsBits
  uint32_t* prefix;            // [kIsHeavyGridWs][words]
  int64_t words;               // per bitmap, padded to 256 B
  int64_t bytes;
};

static IsWs is_carve(void* ws, int64_t n, int64_t b) {
  Carve c{static_cast<char*>(ws)};
  IsWs w{};
  w.head = c.take<int32_t>(n);
  w.next = c.take<int32_t>(b);
  w.clen = c.take<int32_t>(b);
  w.cnt = c.take<int64_t>(b + 1);
  w.mid_row = c.take<int32_t>(b);
  w.heavy_row = c.take<int32_t>(b);
  w.n_class = c.take<int32_t>(2);
  w.temp_bytes = is_temp_bytes(b);
  w.temp = c.take<char>(static_cast<int64_t>(w.temp_bytes));
  w.words = b > kIsLdsBits ? up256((b + 63) / 64 * 8) / 8 : 0;
  w.bitmap = c.take<unsigned long long>(w.words * kIsHeavyGridWs);
  w.prefix = c.take<uint32_t>(w.words * kIsHeavyGridWs);
  w.bytes = c.used;
  return w;
}

// ------------------------------------------------------------------------------------- map
__global__ void is_map_push_kernel(const int64_t* __restrict__ idx, int64_t b, int64_t n,
                                   int32_t* __restrict__ head, int32_t* __restrict__ next,
                                   int32_t* __restrict__ status) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= b) return;
  const int64_t v = idx[p];
  if (v < 0 || v >= n) {
    next[p] = -1;
    atomicOr(status, kIsBadIdx);
    return;
  }
  next[p] = atomicExch(&head[v], static_cast<int32_t>(p));  // head starts at -1: the chain's end
}

__global__ void is_map_len_kernel(const int64_t* __restrict__ idx, int64_t b, int64_t n,
                                  const int32_t* __restrict__ head,
                                  const int32_t* __restrict__ next, int32_t* __restrict__ clen) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= b) return;
  const int64_t v = idx[p];
  int32_t len = 0;
  if (v >= 0 && v < n && head[v] == p)  // the last position pushed walks its id's chain
    for (int64_t q = p; q >= 0 && q < b && len < b; q = next[q]) ++len;
  clen[p] = len;
}

// ------------------------------------------------------------------------- shared by the rows
// A's row of position r: false (and a status bit) for an id or a rowptr span out of range
__device__ __forceinline__ bool is_row_span(const int64_t* __restrict__ rowptr,
                                            const int64_t* __restrict__ idx, int64_t r, int64_t n,
                                            int64_t nnz, int32_t* __restrict__ status, bool report,
                                            int64_t& a, int64_t& e) {
  const int64_t v = idx[r];
  a = e = 0;
  if (v < 0 || v >= n) {
    if (report) atomicOr(status, kIsBadIdx);
    return false;
  }
  a = rowptr[v];
  e = rowptr[v + 1];
  if (a < 0 || e < a || e > nnz) {
    if (report) atomicOr(status, kIsBadGraph);
    a = e = 0;
    return false;
  }
  return true;
}

// entry e of A's row [.., a_end): the number of positions that hold its column id (0: none, the
// entry is dropped) and, in h, the first of them
__device__ __forceinline__ int32_t is_lookup(const int32_t* __restrict__ col,
                                             const int32_t* __restrict__ head,
                                             const int32_t* __restrict__ clen, int64_t e,
                                             int64_t a_end, int64_t n, int64_t b,
                                             int32_t* __restrict__ status, int32_t& h) {
  h = -1;
  if (e >= a_end) return 0;
  const int32_t c = col[e];
  if (c < 0 || c >= n) {
    atomicOr(status, kIsBadGraph);
    return 0;
  }
  h = head[c];
  if (h < 0 || h >= b) {
    h = -1;
    return 0;
  }
  const int32_t len = clen[h];
  return len < 1 ? 1 : (len > b ? static_cast<int32_t>(b) : len);
}

__device__ __forceinline__ int is_wave_incl_scan(int v, int lane) {
  for (int d = 1; d < kWave; d <<= 1) {
    const int o = __shfl_up(v, d, kWave);
    if (lane >= d) v += o;
  }
  return v;
}

// ----------------------------------------------------------------------------------- count
__global__ __launch_bounds__(kIsBlock) void is_count_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t nnz, int64_t n,
    const int64_t* __restrict__ idx, int64_t b, const int32_t* __restrict__ head,
    const int32_t* __restrict__ clen, int64_t* __restrict__ cnt, int32_t* __restrict__ status) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kIsWaves + (threadIdx.x >> 6);
  if (r >= b) return;
  if (r == 0 && lane == 0) cnt[b] = 0;
  int64_t a, e;
  long long sum = 0;
  if (is_row_span(rowptr, idx, r, n, nnz, status, lane == 0, a, e)) {
    for (int64_t c0 = a; c0 < e; c0 += 4 * kWave) {  // four independent lookups in flight
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        int32_t h;
        sum += is_lookup(col, head, clen, c0 + u * kWave + lane, e, n, b, status, h);
      }
    }
  }
  for (int d = kWave / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d, kWave);
  if (lane == 0) cnt[r] = sum;
}

// ---------------------------------------------------------------------------- short rows
// Visits every row: rows above the short limit are queued for their class, short rows are built.
template <bool VAL>
__global__ __launch_bounds__(kIsBlock) void is_short_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, int64_t nnz, int64_t n, const int64_t* __restrict__ idx,
    int64_t b, const int32_t* __restrict__ head, const int32_t* __restrict__ next,
    const int32_t* __restrict__ clen, const int64_t* __restrict__ crp, int32_t* __restrict__ ccol,
    float* __restrict__ cval, int64_t nnz_c, int32_t* __restrict__ mid_row,
    int32_t* __restrict__ heavy_row, int32_t* __restrict__ n_class, int32_t* __restrict__ status) {
  __shared__ unsigned long long keys[kIsWaves][kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kIsWaves + wave;
  int64_t dst = 0, c = 0, a = 0, e = 0;
  if (r < b) {
    dst = crp[r];
    c = crp[r + 1] - dst;
    if (c > kIsShortMax) {
      if (lane == 0) {
        const int k = c <= kIsMidMax ? 0 : 1;
        const int32_t s = atomicAdd(&n_class[k], 1);
        if (s >= 0 && s < b) (k ? heavy_row : mid_row)[s] = static_cast<int32_t>(r);
      }
      c = 0;
    }
    if (c > 0 && !is_row_span(rowptr, idx, r, n, nnz, status, lane == 0, a, e)) c = 0;
  }
  if (c < 0) c = 0;
  unsigned long long* k = keys[wave];
  k[lane] = kIsNoKey;
  __syncthreads();
  if (c > 0) {
    int base = 0;  // keys placed so far
    for (int64_t c0 = a; c0 < e; c0 += kWave) {
      int32_t h;
      const int32_t len = is_lookup(col, head, clen, c0 + lane, e, n, b, status, h);
      if (__ballot(len > 0) == 0) continue;
      const int incl = is_wave_incl_scan(len, lane);
      int o = base + incl - len;
      const unsigned long long ord = static_cast<uint32_t>(c0 + lane - a);
      int32_t p = h;
      for (int t = 0; t < len && p >= 0 && p < b; ++t) {
        if (o < kWave) k[o] = (static_cast<unsigned long long>(static_cast<uint32_t>(p)) << 32) | ord;
        ++o;
        p = next[p];
      }
      base += __shfl(incl, kWave - 1, kWave);
    }
  }
  __syncthreads();
  if (c == 0) return;
  unsigned long long key = k[lane];
  for (int s = 2; s <= kWave; s <<= 1) {  // bitonic sort of the 64 lanes, ascending
    for (int j = s >> 1; j > 0; j >>= 1) {
      const unsigned long long o = __shfl_xor(key, j, kWave);
      const bool up = (lane & s) == 0 || s == kWave;
      const bool low = (lane & j) == 0;
      key = (low == up) ? (key < o ? key : o) : (key > o ? key : o);
    }
  }
  const unsigned long long prev = __shfl_up(key, 1, kWave);
  if (key == kIsNoKey) return;
  if (lane > 0 && (prev >> 32) == (key >> 32)) atomicOr(status, kIsRepeat);
  const int64_t out = dst + lane;
  if (lane < c && out < nnz_c) {
    ccol[out] = static_cast<int32_t>(key >> 32);
    if (VAL) cval[out] = val[a + static_cast<int64_t>(key & 0xffffffffull)];
  }
}

// ------------------------------------------------------------------------------ mid rows
template <bool VAL>
__global__ __launch_bounds__(kIsBlock) void is_mid_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, int64_t nnz, int64_t n, const int64_t* __restrict__ idx,
    int64_t b, const int32_t* __restrict__ head, const int32_t* __restrict__ next,
    const int32_t* __restrict__ clen, const int64_t* __restrict__ crp, int32_t* __restrict__ ccol,
    float* __restrict__ cval, int64_t nnz_c, const int32_t* __restrict__ rows,
    const int32_t* __restrict__ n_rows, int32_t* __restrict__ status) {
  __shared__ unsigned long long keys[kIsMidMax];
  __shared__ int s_total;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  int64_t nr = *n_rows;
  if (nr > b) nr = b;
  for (int64_t q = blockIdx.x; q < nr; q += gridDim.x) {
    const int64_t r = rows[q];
    if (r < 0 || r >= b) continue;
    const int64_t dst = crp[r], c = crp[r + 1] - dst;  // kIsShortMax < c <= kIsMidMax
    if (tid == 0) s_total = 0;
    __syncthreads();
    int64_t a, e;
    if (is_row_span(rowptr, idx, r, n, nnz, status, tid == 0, a, e)) {
      for (int64_t c0 = a + static_cast<int64_t>(wave) * kWave; c0 < e;
           c0 += static_cast<int64_t>(kIsWaves) * kWave) {
        int32_t h;
        const int32_t len = is_lookup(col, head, clen, c0 + lane, e, n, b, status, h);
        if (__ballot(len > 0) == 0) continue;
        const int incl = is_wave_incl_scan(len, lane);
        int base = 0;
        if (lane == kWave - 1) base = atomicAdd(&s_total, incl);  // the wave's keys, in one run
        base = __shfl(base, kWave - 1, kWave);
        int o = base + incl - len;
        const unsigned long long ord = static_cast<uint32_t>(c0 + lane - a);
        int32_t p = h;
        for (int t = 0; t < len && p >= 0 && p < b; ++t) {
          if (o >= 0 && o < kIsMidMax)
            keys[o] = (static_cast<unsigned long long>(static_cast<uint32_t>(p)) << 32) | ord;
          ++o;
          p = next[p];
        }
      }
    }
    __syncthreads();
    int count = s_total;
    if (count > kIsMidMax || count < 0) count = kIsMidMax;
    int sorted = 2;
    while (sorted < count) sorted <<= 1;
    for (int s = count + tid; s < sorted; s += kIsBlock) keys[s] = kIsNoKey;
    __syncthreads();
    for (int k = 2; k <= sorted; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < sorted / 2; t += kIsBlock) {
          const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int hi = lo | j;
          const unsigned long long x = keys[lo], y = keys[hi];
          const bool up = (lo & k) == 0;
          if ((x > y) == up) {
            keys[lo] = y;
            keys[hi] = x;
          }
        }
        __syncthreads();
      }
    }
    for (int s = tid; s < count; s += kIsBlock) {
      const unsigned long long key = keys[s];
      if (s > 0 && (keys[s - 1] >> 32) == (key >> 32)) atomicOr(status, kIsRepeat);
      const int64_t out = dst + s;
      if (s < c && out < nnz_c) {
        ccol[out] = static_cast<int32_t>(key >> 32);
        if (VAL) cval[out] = val[a + static_cast<int64_t>(key & 0xffffffffull)];
      }
    }
    __syncthreads();  // keys and s_total are reused by the next row
  }
}

// ---------------------------------------------------------------------------- heavy rows
// The b-bit bitmap of one workgroup and the exclusive popcount prefix of its 64-bit words: in
// LDS, or in the workspace (read and written at agent scope: other waves of the workgroup read
// the words where the atomics put them, in L2).
template <bool LDS>
struct IsBitmap {
  unsigned long long* bm;
  uint32_t* pre;
  __device__ __forceinline__ unsigned long long set(int64_t w, unsigned long long bits) {
    return atomicOr(&bm[w], bits);
  }
  __device__ __forceinline__ unsigned long long load(int64_t w) const {
    if (LDS) return bm[w];
    return __hip_atomic_load(&bm[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void clear(int64_t w) {
    if (LDS)
      bm[w] = 0ull;
    else
      __hip_atomic_store(&bm[w], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ uint32_t rank_base(int64_t w) const {
    if (LDS) return pre[w];
    return __hip_atomic_load(&pre[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void set_rank_base(int64_t w, uint32_t v) {
    if (LDS)
      pre[w] = v;
    else
      __hip_atomic_store(&pre[w], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the workgroup's global accesses have completed before its other waves go on
  __device__ __forceinline__ void settle() const {
    if (!LDS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
};

template <bool LDS, bool VAL>
__global__ __launch_bounds__(kIsBlock) void is_heavy_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, int64_t nnz, int64_t n, const int64_t* __restrict__ idx,
    int64_t b, const int32_t* __restrict__ head, const int32_t* __restrict__ next,
    const int32_t* __restrict__ clen, const int64_t* __restrict__ crp, int32_t* __restrict__ ccol,
    float* __restrict__ cval, int64_t nnz_c, const int32_t* __restrict__ rows,
    const int32_t* __restrict__ n_rows, unsigned long long* __restrict__ ws_bitmap,
    uint32_t* __restrict__ ws_prefix, int64_t ws_words, int32_t* __restrict__ status) {
  __shared__ unsigned long long s_bm[LDS ? kIsLdsWords : 1];
  __shared__ uint32_t s_pre[LDS ? kIsLdsWords : 1];
  __shared__ int s_min, s_max;  // word indices: < 2^25
  __shared__ unsigned s_run;
  __shared__ int s_wave[kIsWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int64_t words = (b + 63) / 64;
  if (LDS ? words > kIsLdsWords : words > ws_words) return;
  int64_t nr = *n_rows;
  if (nr > b) nr = b;
  if (static_cast<int64_t>(blockIdx.x) >= nr) return;
  IsBitmap<LDS> bm{LDS ? s_bm : ws_bitmap + static_cast<int64_t>(blockIdx.x) * ws_words,
                   LDS ? s_pre : ws_prefix + static_cast<int64_t>(blockIdx.x) * ws_words};
  for (int64_t w = tid; w < words; w += kIsBlock) bm.clear(w);  // whatever the scratch held
  bm.settle();
  for (int64_t q = blockIdx.x; q < nr; q += gridDim.x) {
    const int64_t r = rows[q];
    if (r < 0 || r >= b) continue;
    const int64_t dst = crp[r], end = crp[r + 1];
    if (tid == 0) {
      s_min = static_cast<int>(words);
      s_max = -1;
      s_run = 0;
    }
    __syncthreads();
    int64_t a, e;
    const bool ok = is_row_span(rowptr, idx, r, n, nnz, status, tid == 0, a, e);
    // pass 1: the bits of every kept (entry, position)
    int wmin = static_cast<int>(words), wmax = -1;
    if (ok) {
      for (int64_t c0 = a + static_cast<int64_t>(wave) * kWave; c0 < e;
           c0 += static_cast<int64_t>(kIsWaves) * kWave) {
        int32_t h;
        const int32_t len = is_lookup(col, head, clen, c0 + lane, e, n, b, status, h);
        int32_t p = h;
        for (int t = 0; t < len && p >= 0 && p < b; ++t) {
          const int w = p >> 6;
          const unsigned long long bit = 1ull << (p & 63);
          if (bm.set(w, bit) & bit) atomicOr(status, kIsRepeat);
          wmin = w < wmin ? w : wmin;
          wmax = w > wmax ? w : wmax;
          p = next[p];
        }
      }
    }
    if (wmax >= 0) {
      atomicMin(&s_min, wmin);
      atomicMax(&s_max, wmax);
    }
    bm.settle();
    const int64_t w_lo = s_min, w_hi = s_max;
    // the exclusive popcount prefix of the touched words, 256 words a step
    for (int64_t w0 = w_lo; w0 <= w_hi; w0 += kIsBlock) {
      const int64_t w = w0 + tid;
      const int c = w <= w_hi ? __popcll(bm.load(w)) : 0;
      const int incl = is_wave_incl_scan(c, lane);
      if (lane == kWave - 1) s_wave[wave] = incl;
      __syncthreads();
      int before = 0, step = 0;
      for (int x = 0; x < kIsWaves; ++x) {
        if (x < wave) before += s_wave[x];
        step += s_wave[x];
      }
      const unsigned run = s_run;
      if (w <= w_hi) bm.set_rank_base(w, run + before + incl - c);
      __syncthreads();  // every thread has read s_run and s_wave
      if (tid == 0) s_run = run + step;
    }
    bm.settle();
    // pass 2: every kept (entry, position) to c_rowptr[r] + rank(position)
    if (ok) {
      for (int64_t c0 = a + static_cast<int64_t>(wave) * kWave; c0 < e;
           c0 += static_cast<int64_t>(kIsWaves) * kWave) {
        int32_t h;
        const int32_t len = is_lookup(col, head, clen, c0 + lane, e, n, b, status, h);
        int32_t p = h;
        for (int t = 0; t < len && p >= 0 && p < b; ++t) {
          const int w = p >> 6;
          const unsigned long long below = bm.load(w) & ((1ull << (p & 63)) - 1);
          const int64_t out = dst + bm.rank_base(w) + __popcll(below);
          if (out < end && out < nnz_c) {
            ccol[out] = p;
            if (VAL) cval[out] = val[c0 + lane];
          }
          p = next[p];
        }
      }
    }
    __syncthreads();  // the bitmap is read to here
    for (int64_t w = w_lo + tid; w <= w_hi; w += kIsBlock) bm.clear(w);
    bm.settle();  // and is all zero again; s_min / s_max / s_run are reset by the next row
  }
}

static int is_check_dims(int64_t n, int64_t b) {
  if (n < 0 || b < 0) return GNN_E_ARG;
  if (n >= kIsDimLimit || b >= kIsDimLimit) return GNN_E_UNSUPPORTED;
  return GNN_OK;
}

template <bool VAL>
static void is_launch_fill(const int64_t* rowptr, const int32_t* col, const float* val, int64_t nnz,
                           int64_t n, const int64_t* idx, int64_t b, const IsWs& w,
                           const int64_t* crp, int32_t* ccol, float* cval, int64_t nnz_c,
                           int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(is_short_kernel<VAL>, dim3(blocks(b, kIsWaves)), dim3(kIsBlock), 0, s, rowptr,
                     col, val, nnz, n, idx, b, w.head, w.next, w.clen, crp, ccol, cval, nnz_c,
                     w.mid_row, w.heavy_row, w.n_class, status);
  const int64_t mid_grid = b < kIsMidGrid ? b : kIsMidGrid;
  hipLaunchKernelGGL(is_mid_kernel<VAL>, dim3(static_cast<unsigned>(mid_grid)), dim3(kIsBlock), 0,
                     s, rowptr, col, val, nnz, n, idx, b, w.head, w.next, w.clen, crp, ccol, cval,
                     nnz_c, w.mid_row, w.n_class, status);
  if (b <= kIsLdsBits) {
    const int64_t grid = b < kIsHeavyGridLds ? b : kIsHeavyGridLds;
    hipLaunchKernelGGL((is_heavy_kernel<true, VAL>), dim3(static_cast<unsigned>(grid)),
                       dim3(kIsBlock), 0, s, rowptr, col, val, nnz, n, idx, b, w.head, w.next,
                       w.clen, crp, ccol, cval, nnz_c, w.heavy_row, w.n_class + 1, nullptr, nullptr,
                       static_cast<int64_t>(0), status);
  } else {
    hipLaunchKernelGGL((is_heavy_kernel<false, VAL>), dim3(kIsHeavyGridWs), dim3(kIsBlock), 0, s,
                       rowptr, col, val, nnz, n, idx, b, w.head, w.next, w.clen, crp, ccol, cval,
                       nnz_c, w.heavy_row, w.n_class + 1, w.bitmap, w.prefix, w.words, status);
  }
}

}  // namespace gnn

using namespace gnn;

extern "C" int64_t gnn_induced_subgraph_workspace_bytes(int64_t n, int64_t b) {
  const int rc = is_check_dims(n, b);
  if (rc != GNN_OK) return rc;
  // the terms: the map (4 n + 8 b), O(b) row arrays and rocPRIM's temporaries, and above
  // kIsLdsBits a fixed number of b-bit bitmaps with their word prefixes
  return is_carve(nullptr, n, b).bytes + 256;
}

extern "C" int gnn_induced_subgraph_class_limits(int64_t* short_max, int64_t* mid_max,
                                                 int64_t* lds_bits) {
  if (!short_max || !mid_max || !lds_bits) return GNN_E_ARG;
  *short_max = kIsShortMax;
  *mid_max = kIsMidMax;
  *lds_bits = kIsLdsBits;
  return GNN_OK;
}

extern "C" int gnn_induced_subgraph_map(const int64_t* idx, int64_t b, int64_t n, int32_t* status,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = is_check_dims(n, b);
  if (rc != GNN_OK) return rc;
  if (!status || !workspace || (b > 0 && !idx)) return GNN_E_ARG;
  IsWs w = is_carve(workspace, n, b);
  if (workspace_bytes < w.bytes + 256) return GNN_E_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n > 0) GNN_TRY(hipMemsetAsync(w.head, 0xff, static_cast<size_t>(n) * 4, s));  // all -1
  if (b > 0) {
    hipLaunchKernelGGL(is_map_push_kernel, dim3(blocks(b, 256)), dim3(256), 0, s, idx, b, n,
                       w.head, w.next, status);
    hipLaunchKernelGGL(is_map_len_kernel, dim3(blocks(b, 256)), dim3(256), 0, s, idx, b, n, w.head,
                       w.next, w.clen);
  }
  return launch_status();
}

extern "C" int gnn_induced_subgraph_count(const int64_t* rowptr, const int32_t* col, int64_t nnz,
                                          int64_t n, const int64_t* idx, int64_t b,
                                          int64_t* c_rowptr, int32_t* status, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
  const int rc = is_check_dims(n, b);
  if (rc != GNN_OK) return rc;
  if (nnz < 0 || !rowptr || !c_rowptr || !status || !workspace || (nnz > 0 && !col) ||
      (b > 0 && !idx))
    return GNN_E_ARG;
  IsWs w = is_carve(workspace, n, b);
  if (workspace_bytes < w.bytes + 256) return GNN_E_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (b == 0) {
    GNN_TRY(hipMemsetAsync(c_rowptr, 0, sizeof(int64_t), s));
    return launch_status();
  }
  hipLaunchKernelGGL(is_count_kernel, dim3(blocks(b, kIsWaves)), dim3(kIsBlock), 0, s, rowptr, col,
                     nnz, n, idx, b, w.head, w.clen, w.cnt, status);
  size_t tb = w.temp_bytes;
  GNN_TRY(rocprim::exclusive_scan(w.temp, tb, w.cnt, c_rowptr, static_cast<int64_t>(0),
                                  static_cast<size_t>(b + 1), rocprim::plus<int64_t>(), s));
  return launch_status();
}

extern "C" int gnn_induced_subgraph_fill(const int64_t* rowptr, const int32_t* col,
                                         const float* val, int64_t nnz, int64_t n,
                                         const int64_t* idx, int64_t b, const int64_t* c_rowptr,
                                         int32_t* c_col, float* c_val, int64_t nnz_c,
                                         int32_t* status, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
  const int rc = is_check_dims(n, b);
  if (rc != GNN_OK) return rc;
  if (nnz < 0 || nnz_c < 0 || !rowptr || !c_rowptr || !status || !workspace ||
      (nnz > 0 && !col) || (b > 0 && !idx) || (nnz_c > 0 && !c_col))
    return GNN_E_ARG;
  IsWs w = is_carve(workspace, n, b);
  if (workspace_bytes < w.bytes + 256) return GNN_E_ARG;
  if (nnz_c == 0 || b == 0) return GNN_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  GNN_TRY(hipMemsetAsync(w.n_class, 0, 2 * sizeof(int32_t), s));
  if (val && c_val)
    is_launch_fill<true>(rowptr, col, val, nnz, n, idx, b, w, c_rowptr, c_col, c_val, nnz_c, status,
                         s);
  else
    is_launch_fill<false>(rowptr, col, nullptr, nnz, n, idx, b, w, c_rowptr, c_col, nullptr, nnz_c,
                          status, s);
  return launch_status();
}
