// host.hpp -- host-side plumbing of the C-ABI entries: the workspace carver, launch grids,
// error propagation and the blocking read-back. Included after common.hpp; nothing here is
// seen by device code.
//
// An entry with a multi-piece workspace states its layout once, as a struct XWs and a
// static XWs x_carve(void* ws, dims...) that fills it through Carve and ends with
// w.bytes = c.used. gnn_x_workspace_bytes is x_carve(nullptr, dims).bytes; the entry carves
// once, refuses workspace_bytes < w.bytes before its first device call and hands rocPRIM
// w.temp / w.temp_bytes.
#pragma once

#include "common.hpp"

namespace gnn {

inline int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }

// bump allocator over the caller's workspace. A null base sizes the layout: every pointer
// comes back null and only `used` advances.
struct Carve {
  char* p;
  int64_t used = 0;
  // n elements of T, the piece padded to 256 bytes (n == 0 takes nothing)
  template <class T> T* take(int64_t n) {
    T* r = reinterpret_cast<T*>(p ? p + used : nullptr);
    used += up256(n * static_cast<int64_t>(sizeof(T)));
    return r;
  }
  // exactly `bytes`, unpadded: a layout's slack, or a rocPRIM temporary it never rounded
  void* raw(int64_t bytes) {
    void* r = p ? p + used : nullptr;
    used += bytes;
    return r;
  }
};

// launch grids: ceil(n / per) blocks, and the grid-stride one of 256 threads in [1, 65536]
inline unsigned blocks(int64_t n, int64_t per) { return static_cast<unsigned>((n + per - 1) / per); }
inline unsigned blocks_capped(int64_t n) {
  const int64_t b = (n + 255) / 256;
  return static_cast<unsigned>(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

// a failing step's code is the entry's return code: a hipError_t, or the int of a nested entry
// (hipSuccess == GNN_OK == 0)
#define GNN_TRY(expr)                        \
  do {                                       \
    const int rc_ = static_cast<int>(expr);  \
    if (rc_ != GNN_OK) return rc_;           \
  } while (0)

// count elements from the device, the stream synchronised: the host may read them on return
template <class T> inline int sync_read(const T* dev, T* host, int64_t count, hipStream_t s) {
  GNN_TRY(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, s));
  GNN_TRY(hipStreamSynchronize(s));
  return GNN_OK;
}

}  // namespace gnn
