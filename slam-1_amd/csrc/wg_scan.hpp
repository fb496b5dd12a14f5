// Workgroup rank, exclusive scan and sum of an integer: the one implementation
// of the order-preserving compaction every "keep some of a frame's entries"
// kernel needs (device only).
//
// Contract of wg_rank, wg_exscan and wg_sum<WG> (WG = lanes of the workgroup):
//  * every lane of the workgroup calls it, from uniform control flow;
//  * the LDS argument is WG / 64 ints;
//  * there are exactly two workgroup barriers: one after the wave totals are
//    written, one after they are read -- so the buffer is reusable on return,
//    and whatever a lane wrote to LDS before the call is visible to all lanes
//    after it;
//  * `total` is uniform.  A caller that walks a frame in chunks of WG keeps its
//    running offset in a uniform register (carry += total), never in LDS.
#pragma once

#include "common.hpp"

namespace {

// min(max(v, 0), cap): a count read from device memory, made safe to loop over
__device__ __forceinline__ int clamp_count(int v, int cap) { return min(max(v, 0), cap); }

// Exclusive rank of this lane among the lanes with `keep`, in lane order, and
// the number of such lanes in the workgroup.
template <int WG>
__device__ __forceinline__ int wg_rank(bool keep, int* wave_tot, int& total) {
  static_assert(WG % kWave == 0, "whole waves");
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wave_tot[wid] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < WG / kWave; ++w) {
    off += w < wid ? wave_tot[w] : 0;
    tot += wave_tot[w];
  }
  __syncthreads();  // wave_tot may be written again
  total = tot;
  return off + __popcll(m & ((1ull << lane) - 1ull));
}

// Sum of v over the lanes before this one, and over the workgroup.
template <int WG>
__device__ __forceinline__ int wg_exscan(int v, int* wave_tot, int& total) {
  static_assert(WG % kWave == 0, "whole waves");
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
  int incl = v;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int o = __shfl_up(incl, off, kWave);
    if (lane >= off) incl += o;
  }
  if (lane == kWave - 1) wave_tot[wid] = incl;
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < WG / kWave; ++w) {
    off += w < wid ? wave_tot[w] : 0;
    tot += wave_tot[w];
  }
  __syncthreads();  // wave_tot may be written again
  total = tot;
  return off + incl - v;
}

// Sum of v over the workgroup (every lane gets it).
template <int WG>
__device__ __forceinline__ int wg_sum(int v, int* red) {
  static_assert(WG % kWave == 0, "whole waves");
  const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  if (lane == 0) red[wid] = v;
  __syncthreads();
  int s = 0;
  for (int w = 0; w < WG / kWave; ++w) s += red[w];
  __syncthreads();  // red may be written again
  return s;
}

}  // namespace
