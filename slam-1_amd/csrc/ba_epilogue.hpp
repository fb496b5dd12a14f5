// The epilogue of every camera solve (k_solve_blk in ba_solve.hip,
// k_tl2_epilogue and k_tl3_flow in ba_tiled.hip).
#pragma once

#include "ba_common.hpp"
#include "ba_layout.hpp"
#include "ba_project.hpp"

namespace {

// Inputs of the epilogue: camera gradient, Gram diagonal, live cameras and the
// per-camera cost partials (global memory in the tiled solves, LDS copies prefetched at
// kernel start in k_solve_blk so their latency is off the critical path).
struct EpiSrc {
  const double *g, *dU, *cam, *costc;
};
#ifdef SLAM_FLOW_PROFILE
// the dataflow solve's epilogue: start, x staged, pc / cost reduced, cameras prepared
// (no relocatable device code: every file that includes this header has its
// own copy.  Only the GLOBAL epilogue stamps it, and only ba_tiled.hip instantiates
// that one, so its slam_flow_epi_stamps reads the copy that k_tl3_flow /
// k_tl2_epilogue write.)
__device__ unsigned long long g_flow_epi[4];
#endif

// Shared epilogue: camera step, trial cameras, predicted reduction of the camera
// part, LM cost at the live parameters.  GLOBAL (the tiled solves, 9C up to
// 8192): the inputs are read from memory, so every thread issues its loads in
// groups of 8 before using them (the per-thread order of the pc sum is the
// same), and the per-camera cost is summed by all threads (strided, then the
// fixed tree of block_sum2) instead of by thread 0 alone -- at C5 the serial
// forms were ~18 dependent memory round trips per thread plus 500 dependent
// loads and adds.
__device__ __forceinline__ void block_sum2(double& a, double& b, double* lds) {
  // deterministic: fixed shuffle tree then fixed LDS order (lds: 2 x 16 doubles)
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    lds[wid] = a;
    lds[16 + wid] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
    a = 0.0;
    b = 0.0;
    for (int w = 0; w < nw; ++w) {
      a += lds[w];
      b += lds[16 + w];
    }
  }
  __syncthreads();
}

template <bool GLOBAL = false>
__device__ void solve_epilogue(const slam_ba_problem& p, const double* x, bool ok, double* red,
                               const EpiSrc& e, int fail_code = 1) {
  const int C9 = 9 * p.n_cams, t = threadIdx.x;
  double* state = p.state;
  const double lam = state[SLAM_BA_ST_LAMBDA];
  const int cur = cur_of(state);
  double pc = 0.0, cost = 0.0;
  if constexpr (GLOBAL) {
    const int nt = blockDim.x;
    for (int i0 = t; i0 < C9; i0 += 8 * nt) {
      double xv[8], cv[8], uv[8], gv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int i = min(i0 + q * nt, C9 - 1);
        xv[q] = x[i];
        cv[q] = e.cam[i];
        uv[q] = e.dU[i];
        gv[q] = e.g[i];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int i = i0 + q * nt;
        if (i < C9) {
          const double d = ok ? xv[q] : 0.0;
          p.delta_c[i] = d;
          p.cams[1 - cur][i] = cv[q] + d;
          pc += d * (lam * clampd(uv[q]) * d + gv[q]);
        }
      }
    }
    for (int c = t; c < p.n_cams; c += nt) cost += e.costc[c];
    block_sum2(pc, cost, red);  // (its barriers also publish the trial cameras to the WG)
#ifdef SLAM_FLOW_PROFILE
    if (t == 0) g_flow_epi[2] = wall_clock64();
#endif
  } else {
    for (int i = t; i < C9; i += blockDim.x) {
      const double d = ok ? x[i] : 0.0;
      p.delta_c[i] = d;
      p.cams[1 - cur][i] = e.cam[i] + d;
      pc += d * (lam * clampd(e.dU[i]) * d + e.g[i]);
    }
    pc = block_sum(pc, red);  // (its barriers also publish the trial cameras to the WG)
    if (t == 0)
      for (int c = 0; c < p.n_cams; ++c) cost += e.costc[c];
  }
  for (int c = t; c < p.n_cams; c += blockDim.x)
    cam_prep(p.cams[1 - cur] + 9 * c, p.camrec[1 - cur] + kCamRec * c);
#ifdef SLAM_FLOW_PROFILE
  if (GLOBAL) {
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (t == 0) g_flow_epi[3] = wall_clock64();
  }
#endif
  if (t == 0) {
    state[SLAM_BA_ST_COST] = 0.5 * cost;
    state[SLAM_BA_ST_PRED_CAM] = 0.5 * pc;
    state[SLAM_BA_ST_CHOL_FAIL] = ok ? 0.0 : (double)fail_code;
    if (!ok && fail_code == 2) state[SLAM_BA_ST_SOLVE_FAULT] += 1.0;
  }
}

}  // namespace
