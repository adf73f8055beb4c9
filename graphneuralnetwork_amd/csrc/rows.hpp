// rows.hpp -- element types of a gathered feature table and one lane's share of a row, shared
// by the SpMM (spmm_kernels.hpp) and GraphSAGE (sage_kernels.hpp) gathers.
//
// A table holds float, or bf16_t: 2-byte storage, the high half of an fp32, so the widening is
// exact and order-preserving (a shift or a mask). Row<T, VW> is what one lane loads of a row:
// Raw is what the load leaves in registers (the bf16 pairs stay packed until the use), f32()
// widens it to the VW floats all arithmetic runs on.
#pragma once

#include "common.hpp"

namespace gnn {

struct bf16_t { uint16_t bits; };  // bf16 storage; fp32 value = bits << 16
typedef float f8 __attribute__((ext_vector_type(8)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

// 8 floats per lane (the accumulators of a lane that holds 8 bf16 of a row): moved as two
// 16-B pieces, so the fp32 operands need no more than the 16-B alignment of the f4 path
template <> struct Vec<8> { typedef f8 T; };
template <>
__device__ __forceinline__ f8 vload<8>(const float* p) {
  const f4 a = *reinterpret_cast<const f4*>(p), b = *reinterpret_cast<const f4*>(p + 4);
  return f8{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
}
template <>
__device__ __forceinline__ void vstore<8>(float* p, f8 v) {
  *reinterpret_cast<f4*>(p) = f4{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f4*>(p + 4) = f4{v[4], v[5], v[6], v[7]};
}
__device__ __forceinline__ f8 shfl_xor_f(f8 v, int m) {
  f8 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = __shfl_xor(v[i], m, kWave);
  return r;
}
__device__ __forceinline__ float vget(f8 v, int i) { return v[i]; }
__device__ __forceinline__ void vset(f8& v, int i, float x) { v[i] = x; }

// One lane's VW elements of a row of T. ninf(): VW elements of -inf (the identity of a max).
template <typename T, int VW> struct Row;
template <int VW> struct Row<float, VW> {
  typedef typename Vec<VW>::T Raw;
  static __device__ __forceinline__ Raw load(const float* p) { return vload<VW>(p); }
  static __device__ __forceinline__ Raw zero() { return vzero<VW>(); }
  static __device__ __forceinline__ Raw ninf() { return Raw(-INFINITY); }
  static __device__ __forceinline__ typename Vec<VW>::T f32(Raw r) { return r; }
};
__device__ __forceinline__ float bf16_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
constexpr uint32_t kBf16NinfPair = 0xff80ff80u;  // two bf16 -inf
template <> struct Row<bf16_t, 1> {  // any width, any 2-B aligned view
  typedef uint32_t Raw;
  static __device__ __forceinline__ Raw load(const bf16_t* p) { return p->bits; }
  static __device__ __forceinline__ Raw zero() { return 0u; }
  static __device__ __forceinline__ Raw ninf() { return 0xff80u; }
  static __device__ __forceinline__ float f32(Raw r) { return bf16_lo(r); }
};
template <> struct Row<bf16_t, 4> {
  typedef u2 Raw;
  static __device__ __forceinline__ Raw load(const bf16_t* p) {
    return *reinterpret_cast<const u2*>(p);
  }
  static __device__ __forceinline__ Raw zero() { return u2{0u, 0u}; }
  static __device__ __forceinline__ Raw ninf() { return u2{kBf16NinfPair, kBf16NinfPair}; }
  static __device__ __forceinline__ f4 f32(Raw r) {
    return f4{bf16_lo(r.x), bf16_hi(r.x), bf16_lo(r.y), bf16_hi(r.y)};
  }
};
template <> struct Row<bf16_t, 8> {
  typedef u4 Raw;
  static __device__ __forceinline__ Raw load(const bf16_t* p) {
    return *reinterpret_cast<const u4*>(p);
  }
  static __device__ __forceinline__ Raw zero() { return u4{0u, 0u, 0u, 0u}; }
  static __device__ __forceinline__ Raw ninf() {
    return u4{kBf16NinfPair, kBf16NinfPair, kBf16NinfPair, kBf16NinfPair};
  }
  static __device__ __forceinline__ f8 f32(Raw r) {
    return f8{bf16_lo(r.x), bf16_hi(r.x), bf16_lo(r.y), bf16_hi(r.y),
              bf16_lo(r.z), bf16_hi(r.z), bf16_lo(r.w), bf16_hi(r.w)};
  }
};

}  // namespace gnn
