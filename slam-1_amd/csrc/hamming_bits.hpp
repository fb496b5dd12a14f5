// Device helpers shared by the Hamming matchers (hamming.hip: brute force,
// guided.hip: windowed search): 256-bit Hamming distance on 8 dwords and the
// branch-free running top-2 on packed keys dist << 16 | index.
#pragma once

#include "common.hpp"

namespace {

// popcount-accumulate: v_bcnt_u32_b32 d, x, acc (one VALU op per dword; the
// compiler would otherwise split the sum into v_add3 trees)
__device__ __forceinline__ uint32_t bcnt_acc(uint32_t x, uint32_t acc) {
  uint32_t d;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(d) : "v"(x), "v"(acc));
  return d;
}

__device__ __forceinline__ uint32_t hd8(const uint32_t (&a)[8], const uint4& x,
                                        const uint4& y) {
  uint32_t d = bcnt_acc(a[0] ^ x.x, 0u);
  d = bcnt_acc(a[1] ^ x.y, d);
  d = bcnt_acc(a[2] ^ x.z, d);
  d = bcnt_acc(a[3] ^ x.w, d);
  d = bcnt_acc(a[4] ^ y.x, d);
  d = bcnt_acc(a[5] ^ y.y, d);
  d = bcnt_acc(a[6] ^ y.z, d);
  d = bcnt_acc(a[7] ^ y.w, d);
  return d;
}

__device__ __forceinline__ uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) {
  // LLVM folds this min/max pattern into a single v_med3_u32.
  return max(min(a, b), min(max(a, b), c));
}

// Top-2 keys (k1 <= k2) merged with another top-2 (a1 <= a2).
__device__ __forceinline__ void merge2(uint32_t& k1, uint32_t& k2, uint32_t a1, uint32_t a2) {
  const uint32_t n1 = min(k1, a1);
  const uint32_t n2 = min(max(k1, a1), min(k2, a2));
  k1 = n1;
  k2 = n2;
}

}  // namespace
