// What the BA translation units share: the batch descriptor, the solver-side
// constants and reductions, the sc1 / ticket hand-off, the layout of sys, and
// the host functions through which one BA file reaches another's launches.
#pragma once

#include "common.hpp"

#include <cmath>

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr double kDiagMin = 1e-6, kDiagMax = 1e32;

// Batched LM: independent problems (local-BA windows) advance through one set
// of launches, one problem per blockIdx.y; each keeps its own buffers and LM
// state, so the iterates of a batched problem equal its solo iterates.  The
// problem descriptors travel by value in the kernel arguments (16 x 408 B).
constexpr int kBaMaxBatch = SLAM_BA_MAX_BATCH;
struct BaBatch {
  slam_ba_problem p[kBaMaxBatch];
};
#define BA_PROB(b) const slam_ba_problem& p = (b).p[blockIdx.y]
// the batch travels by value in the kernel arguments: 16 x 408 B,
// beyond the traditional 4 KB; ROCm 7.2 takes it (tests/test_ba.py launches 16)
static_assert(sizeof(slam_ba_problem) == 408, "slam_ba_problem grew: re-check the kernarg size");
static_assert(sizeof(BaBatch) <= 16 * 408, "BaBatch kernel argument size");

// The LM kernels are short and latency-bound and usually share their CUs with
// the (throughput-bound) ORB workgroups of the concurrent tracking stream: they
// raise their waves' issue priority so their dependent chains are issued first
// and the ORB waves fill the gaps.
__device__ __forceinline__ void lm_wave_priority() { __builtin_amdgcn_s_setprio(3); }

__device__ __forceinline__ double block_sum(double v, double* lds) {
  // deterministic: fixed shuffle tree then fixed LDS order
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) lds[wid] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
    for (int w = 0; w < nw; ++w) s += lds[w];
  }
  __syncthreads();
  return s;  // valid on thread 0
}

__device__ __forceinline__ int cur_of(const double* state) {
  return state[SLAM_BA_ST_CUR] != 0.0 ? 1 : 0;
}

__device__ __forceinline__ double clampd(double d) { return fmin(fmax(d, kDiagMin), kDiagMax); }

// Layout of sys (the buffer all-reduced across ranks).  Dense (9C <= 120, the
// one-workgroup solver): S [(9C)^2] row-major, all C(C+1)/2 blocks listed.
// Packed (larger systems, tiled solver): only the listed upper blocks
// (diagonal + camera pairs with common points), 81 doubles each, row-major
// (rows of c1, columns of c2).  Then b, g, diag U [9C] each and cost [C].
constexpr int kDenseMaxN = 120;
__host__ __device__ __forceinline__ bool sys_packed(int n_cams) { return 9 * n_cams > kDenseMaxN; }
__host__ __device__ __forceinline__ long long sys_vec_off(int n_cams, int n_blocks) {
  return sys_packed(n_cams) ? 81ll * n_blocks : 81ll * n_cams * n_cams;
}
constexpr int kLdsMaxN = kDenseMaxN;  // k_solve_blk keeps the system in LDS up to 9C = 120

// Cross-workgroup hand-off inside one launch (ticket pattern): the partials
// are stored and loaded with agent-scope relaxed atomics, i.e. write-through
// `sc1` stores and `sc1` loads that bypass the per-XCD L2, so no L2-wide
// release/acquire fence is needed (MI355X_MICROARCH.md, correctness table).
__device__ __forceinline__ void st_sc1(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_sc1(const double* p) {
  return __hip_atomic_load(const_cast<double*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned ticket_add(uint32_t* p) {
  return __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ticket_reset(uint32_t* p) {
  __hip_atomic_store(p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr int kBS = 256;   // block size of the element-wise kernels

}  // namespace

// Host functions that cross the BA files.  Kernels stay private to their file
// (anonymous namespace, no relocatable device code).  (BaBatch itself stays in
// the anonymous namespace above: it is part of the kernels' mangled names.)
namespace slam {

// Descriptor batch of problems [i0, i0 + n) (n <= kBaMaxBatch) and the launch
// extents that cover the largest of them.
struct Launch {
  BaBatch b;
  int n, max_grps, max_blocks, max_sgrps, mode;
  size_t solve_lds;
  bool dense;
  bool robust;  // a problem of the batch has loss != 0: the ROBUST kernels (each branches per problem)
  bool fused;   // the camera solve assembles (k_solve_blk<true>, no k_assemble launch): slam_ba_iterate_batch only
};

size_t solve_blk_lds(int n_cams);                      // ba_solve.hip: LDS bytes of k_solve_blk
int launch_solve_blk(const Launch& L, hipStream_t s);  // ba_solve.hip: k_solve_blk<L.fused>
int launch_solve_tiled(const slam_ba_problem& p, hipStream_t s);  // ba_tiled.hip: k_tl3_flow or k_tl2_*
int make_launch(const slam_ba_problem* probs, int n, Launch* L);  // ba.hip (ba_cov.hip builds through it)
int launch_build(const Launch& L, hipStream_t s);                 // ba.hip: lineariser + k_assemble (not when L.fused)

}  // namespace slam
