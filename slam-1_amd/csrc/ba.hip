// Levenberg-Marquardt bundle adjustment (BAL model) for gfx950.
//
// Replaces the reference's BAL block (/root/reference/BundleAdjustment.py:287-402:
// rotate, project, objective with its two >5000 px clamps, the 2x12 sparsity
// and scipy least_squares TRF) with LM on the normal equations, all state on
// the device so a fixed number of iterations runs with no host round trip.
//
// One LM iteration = 4 launches (local BA).  This file holds the
// linearisers with the fold, k_assemble, the point step and the decision, and
// the LM entry points; the camera solve is in ba_solve.hip (k_solve_blk) and
// ba_tiled.hip (k_tl3_flow / k_tl2_*), the covariance in ba_cov.hip.  Shared:
// ba_common.hpp (batch descriptor, solver-side helpers, the host functions that
// cross the files), ba_layout.hpp, ba_project.hpp (cam_prep and the
// per-observation projection), ba_epilogue.hpp (solve epilogue), dpp_fmac.hpp
// (fused DPP broadcast FMAs).
//   k_linearize     point group -> residuals + Jacobians, V*_p, e_p = V*^-1 g_p,
//                                  W_o = Jc^T Jp, u_o = Jp e_p, and the group's
//                                  slot partials of the reduced camera system:
//                                  per camera U - sum Y W^T, Jc^T r, Jc^T u;
//                                  per camera pair sum Y_o1 W_o2^T
//   k_assemble      block  -> S = sum of its slot partials in group order,
//                             b = -Jc^T r - Jc^T u, g, diag U, cost
//   (all-reduce of sys over ranks happens here for multi-GPU)
//   k_solve_blk     1 WG   -> damp, blocked LDL^T (MFMA trailing updates), camera  [ba_solve.hip]
//                             step, pred_cam, trial cameras (tiled k_tl3_flow / k_tl2_* for 9C > 120)  [ba_tiled.hip]
//                             (slam_ba_iterate_batch, windows of few partial rows: k_solve_blk<true>
//                             sums the partials itself, in k_assemble's order, and k_assemble is not launched)
//   k_back_trial    point group -> point step, trial points, trial |r|^2 and
//                                  pred partials; the last group sums them into
//                                  small (and, single rank, decides)
//   (all-reduce of small over ranks, then k_decide)
//   k_decide        1 lane -> rho, accept/reject, lambda update, buffer swap
#include "ba_common.hpp"
#include "ba_epilogue.hpp"
#include "ba_layout.hpp"
#include "ba_project.hpp"
#include "dpp_fmac.hpp"

using slam::Launch;
using slam::launch_build;
using slam::make_launch;

namespace {

constexpr double kLamMin = 1e-16, kLamMax = 1e32;

// The batched per-observation / per-block launches (grid x = the problem's
// workgroups, y = problem) with 8k problems: workgroups are dealt round-robin
// over the 8 XCDs (for speed only; nothing depends on it), so the linear
// workgroup id is remapped to keep each problem's workgroups on one XCD --
// problem w's observations, points and partial rows stay in that XCD's L2
// from k_lin_mfma through k_assemble to k_back_trial.  The same (x, problem)
// pairs run either way, so results do not change.
#ifndef SLAM_BA_XCD
#define SLAM_BA_XCD 1
#endif
__device__ __forceinline__ int2 ba_xcd_map() {
  const int gx = (int)gridDim.x, n = (int)gridDim.y;
  if (!SLAM_BA_XCD || n < 8 || (n & 7)) return int2{(int)blockIdx.x, (int)blockIdx.y};
  const int lin = (int)blockIdx.y * gx + (int)blockIdx.x;
  const int xcd = lin & 7, slot = lin >> 3;  // n gx / 8 slots per XCD: its n / 8 problems
  const int wi = slot / gx;
  return int2{slot - wi * gx, xcd + 8 * wi};
}
#define BA_PROB_X(b)                 \
  const int2 bw_ = ba_xcd_map();     \
  const int bx = bw_.x;              \
  const slam_ba_problem& p = (b).p[bw_.y]
// ---------------------------------------------------------------- standalone
__global__ __launch_bounds__(kBS) void k_residual(const double* __restrict__ cams,
                                                  const double* __restrict__ pts,
                                                  const int32_t* __restrict__ ci,
                                                  const int32_t* __restrict__ pi,
                                                  const double* __restrict__ qs, int n_obs,
                                                  double* __restrict__ resid,
                                                  double* __restrict__ jac) {
  const int o = blockIdx.x * kBS + threadIdx.x;
  if (o >= n_obs) return;
  double r[2], J[2][12];
  if (jac) {
    reproject<true>(cams + 9 * ci[o], pts + 3 * pi[o], qs + 2 * o, r, J);
    clamp_rows<true>(r, J);
    for (int a = 0; a < 2; ++a)
      for (int k = 0; k < 12; ++k) jac[(size_t)o * 24 + a * 12 + k] = J[a][k];
  } else {
    reproject<false>(cams + 9 * ci[o], pts + 3 * pi[o], qs + 2 * o, r, J);
    clamp_rows<false>(r, J);
  }
  resid[2 * o] = r[0];
  resid[2 * o + 1] = r[1];
}

// ---------------------------------------------------------------- LM kernels


// Per point: V = sum Jp^T Jp and g = -sum Jp^T r over its observations, in
// observation order (pt_acc per observation row), then V* = V + lam diag(V)
// (diag clamped), V*^-1 by cofactors and e = V*^-1 g (pt_schur).  The
// linearisers and k_back_trial run the same operations in the same order on
// every value (k_lin_mfma: one lane per component, pt_comp below), so the back
// substitution sees bit-identical V*^-1, e, g, diag.
struct PtSchur {
  double V00 = 0, V01 = 0, V02 = 0, V11 = 0, V12 = 0, V22 = 0, g0 = 0, g1 = 0, g2 = 0;
  double d[3], iv[6], e[3];
  __device__ __forceinline__ void acc(double j0, double j1, double j2, double rr) {
    V00 += j0 * j0; V01 += j0 * j1; V02 += j0 * j2;
    V11 += j1 * j1; V12 += j1 * j2; V22 += j2 * j2;
    g0 -= j0 * rr; g1 -= j1 * rr; g2 -= j2 * rr;
  }
  __device__ __forceinline__ void solve(double lam);
};
__device__ __forceinline__ void PtSchur::solve(double lam) {
  d[0] = clampd(V00); d[1] = clampd(V11); d[2] = clampd(V22);
  const double a00 = V00 + lam * d[0], a11 = V11 + lam * d[1], a22 = V22 + lam * d[2];
  const double a01 = V01, a02 = V02, a12 = V12;
  const double c00 = a11 * a22 - a12 * a12;
  const double c01 = a02 * a12 - a01 * a22;
  const double c02 = a01 * a12 - a02 * a11;
  const double c11 = a00 * a22 - a02 * a02;
  const double c12 = a01 * a02 - a00 * a12;
  const double c22 = a00 * a11 - a01 * a01;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  const double id = det != 0.0 ? 1.0 / det : 0.0;
  iv[0] = c00 * id; iv[1] = c01 * id; iv[2] = c02 * id;
  iv[3] = c11 * id; iv[4] = c12 * id; iv[5] = c22 * id;
  e[0] = iv[0] * g0 + iv[1] * g1 + iv[2] * g2;
  e[1] = iv[1] * g0 + iv[3] * g1 + iv[4] * g2;
  e[2] = iv[2] * g0 + iv[4] * g1 + iv[5] * g2;
}

// Component j of a point's (V00 V01 V02 V11 V12 V22 g0 g1 g2) over its
// observations [kb, ke), rows a = 0, 1 of each in turn: the chain of rounded
// products and sums PtSchur::acc runs for that component (g -= x y is
// g += (-x) y, exactly), so a lane per (point, component) gives the bits one
// lane per point gives.  jr: [8][stride], rows 0..5 Jp (2 x 3), 6..7 r.  The
// operands of 4 observations are loaded before their sums are taken.
__device__ __forceinline__ double pt_comp(const double* jr, int stride, int kb, int ke, int j) {
  const int ia = j < 3 ? 0 : j < 5 ? 1 : j < 6 ? 2 : j - 6;
  const int ib = j < 3 ? j : j < 5 ? j - 2 : 2;
  const bool isg = j >= 6;
  const double* xr[2] = {jr + ia * stride, jr + (3 + ia) * stride};
  const double* yr[2] = {jr + (isg ? 6 : ib) * stride, jr + (isg ? 7 : 3 + ib) * stride};
  double v = 0.0;
  for (int k = kb; k < ke; k += 4) {
    double x[4][2], y[4][2];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kk = min(k + u, ke - 1);
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        x[u][a] = xr[a][kk];
        y[u][a] = yr[a][kk];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (k + u >= ke) break;
#pragma unroll
      for (int a = 0; a < 2; ++a) v += (isg ? -x[u][a] : x[u][a]) * y[u][a];
    }
  }
  return v;
}

// Point groups: a workgroup owns the contiguous observation range of a group
// of whole points (observations are sorted by point), at most kGrp of them.
constexpr int kGrp = 128;
constexpr int kLinWG = 256;  // k_linearize: obs / point phases use kGrp lanes, slot phase all
constexpr int kSlotLds = 128;  // slot ranges staged in LDS (larger groups read them from memory)
constexpr int kPairLds = 1024; // observation pairs staged in LDS (ditto)

// LDS of k_linearize (65.5 KiB: leaves room for a co-resident ORB workgroup)
struct LinLds {
  double jc[kGrp][18];  // Jc rows (2 x 9)
  double w[kGrp][27];   // W = Jc^T Jp [i][c]; before phase 3: Jp (6), r (2)
  double ru[kGrp][4];   // r0 r1 u0 u1
  double pt[kGrp][9];   // per group point: e (3), V*^-1 (i00 i01 i02 i11 i12 i22)
  int lpt[kGrp];        // group-local point of each observation
  int cobs[kGrp];       // the group's camera-slot observation lists
  int cptr[kSlotLds];   // camera-slot ranges in cobs (when the group has < kSlotLds slots)
  int bptr[kSlotLds];   // block-slot ranges in pairs
  int pairs[kPairLds];  // the group's observation pairs (when <= kPairLds)
  unsigned fx[kGrp];    // held-parameter mask of each observation's camera (cam_fixed only)
  double rho[kGrp];     // delta^2 rho(z) of each observation (robust loss only)
};

// Y_o row i (= W_o row i times V*^-1, V*^-1 symmetric) of a group observation
__device__ __forceinline__ void y_row(const double* W, const double* Vi, int i, double y[3]) {
  const double a = W[3 * i], b = W[3 * i + 1], c = W[3 * i + 2];
  y[0] = a * Vi[0] + b * Vi[1] + c * Vi[2];
  y[1] = a * Vi[1] + b * Vi[3] + c * Vi[4];
  y[2] = a * Vi[2] + b * Vi[4] + c * Vi[5];
}

// Linearisation, point elimination and the group's share of the reduced camera
// system, one workgroup per point group:
//   per observation: residual and 2x12 Jacobian (BundleAdjustment.py:317-350
//     + analytic derivative) -> LDS;
//   per point: V = sum Jp^T Jp, g = -sum Jp^T r, V* = V + lam diag(V),
//     V*^-1 (cofactors), e = V*^-1 g;
//   per observation: W = Jc^T Jp, u = Jp e -> LDS;
//   per slot row (a lane owns row i of one slot; slots from the planner):
//     camera slot (c):      U - sum_o Y_o W_o^T, Jc^T r, Jc^T u, diag U, |r|^2
//                           over the group's observations of camera c;
//     block slot (c1 <= c2): sum Y_o1 W_o2^T over the group's observation pairs
//                           o1 < o2 of one point with cameras c1, c2.
// Everything stays in LDS between the phases; only the slot partials (and the
// per-point data the back substitution needs) are written.
// Slot partials of one group (see k_linearize): a lane owns row i of one slot
// (405 lanes' worth at C3: two rounds of the workgroup).
// cptr / bptr: slot ranges (minus coff / boff) into the group's camera-slot
// observations (L.cobs) and observation pairs.
template <bool ROBUST>
__device__ __forceinline__ void lin_slots(const slam_ba_problem& p, LinLds& L, int cs0, int ncs,
                                          int bs0, int nbs, const int* cptr, int coff,
                                          const int* bptr, int boff, const int* pairs) {
  const int t = threadIdx.x;
  const int* cobs = L.cobs;
  const bool robust = ROBUST && p.loss != 0;  // uniform: the cost term is delta^2 rho(z) (L.rho), not |r~|^2
  for (int item = t; item < 9 * (ncs + nbs); item += kLinWG) {
    const int sl = item / 9, i = item - 9 * sl;
    double acc[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[j] = 0.0;
    if (sl < ncs) {
      const int s = cs0 + sl;
      double vr = 0.0, vu = 0.0, vd = 0.0, cost = 0.0;
      // the next observation's index and point are fetched one iteration
      // ahead, so each iteration waits on one LDS round trip, not three
      const int qb = cptr[sl] - coff, qe = cptr[sl + 1] - coff;
      int k = cobs[qb < qe ? qb : 0], lk = L.lpt[k];
      for (int q = qb; q < qe; ++q) {
        const int kn = cobs[q + 1 < qe ? q + 1 : q], lkn = L.lpt[kn];
        const double* jc = L.jc[k];
        const double* W = L.w[k];
        double y[3];
        y_row(W, L.pt[lk] + 3, i, y);
        const double a0 = jc[i], a1 = jc[9 + i];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
          const double u = __builtin_fma(a0, jc[j], a1 * jc[9 + j]);
          const double v = __builtin_fma(y[0], W[3 * j], __builtin_fma(y[1], W[3 * j + 1], y[2] * W[3 * j + 2]));
          acc[j] += u - v;
        }
        const double r0 = L.ru[k][0], r1 = L.ru[k][1];
        vr = __builtin_fma(a0, r0, __builtin_fma(a1, r1, vr));
        vu = __builtin_fma(a0, L.ru[k][2], __builtin_fma(a1, L.ru[k][3], vu));
        vd = __builtin_fma(a0, a0, __builtin_fma(a1, a1, vd));
        if (robust) cost += L.rho[k];
        else cost = __builtin_fma(r0, r0, __builtin_fma(r1, r1, cost));
        k = kn;
        lk = lkn;
      }
      double* out = p.cpart + (size_t)p.cslot_row[s] * kCPart;
#pragma unroll
      for (int j = 0; j < 9; ++j) out[9 * i + j] = acc[j];
      out[81 + i] = vr;
      out[90 + i] = vu;
      out[99 + i] = vd;
      if (i == 0) out[108] = cost;
    } else {
      const int sb = sl - ncs, s = bs0 + sb;
      const int qb = bptr[sb] - boff, qe = bptr[sb + 1] - boff;
      int pr = pairs[qb < qe ? qb : 0], lk = L.lpt[pr & 0xffff];
      for (int q = qb; q < qe; ++q) {
        const int prn = pairs[q + 1 < qe ? q + 1 : q], lkn = L.lpt[prn & 0xffff];
        const int k1 = pr & 0xffff, k2 = pr >> 16;
        double y[3];
        y_row(L.w[k1], L.pt[lk] + 3, i, y);
        const double* W2 = L.w[k2];
#pragma unroll
        for (int j = 0; j < 9; ++j)
          acc[j] = __builtin_fma(y[0], W2[3 * j], __builtin_fma(y[1], W2[3 * j + 1], __builtin_fma(y[2], W2[3 * j + 2], acc[j])));
        pr = prn;
        lk = lkn;
      }
      double* out = p.bpart + (size_t)p.bslot_row[s] * 81;
#pragma unroll
      for (int j = 0; j < 9; ++j) out[9 * i + j] = acc[j];
    }
  }
}

template <bool ROBUST>  // as k_lin_mfma
__global__ __launch_bounds__(kLinWG) void k_linearize(BaBatch bat) {
  BA_PROB_X(bat);
  const int g = bx;
  if (g >= p.n_grps) return;  // batch: grid.x covers the largest problem
  lm_wave_priority();
  __shared__ LinLds L;
  const int p0 = p.grp_ptr[g], p1 = p.grp_ptr[g + 1];
  const int o0 = p.pt_ptr[p0], o1 = p.pt_ptr[p1];
  const int t = threadIdx.x;
  const int o = o0 + t;
  const bool has = t < kGrp && o < o1;
  const int cur = cur_of(p.state);
  // slot lists of this group -> LDS (their loads overlap the projections)
  const int cs0 = p.grp_cslot[g], ncs = p.grp_cslot[g + 1] - cs0;
  const int bs0 = p.grp_bslot[g], nbs = p.grp_bslot[g + 1] - bs0;
  const int cb0 = p.cslot_obs_ptr[cs0], pb0 = p.bslot_pair_ptr[bs0];
  const int npairs = p.bslot_pair_ptr[bs0 + nbs] - pb0;
  const bool fit_c = ncs < kSlotLds, fit_b = nbs < kSlotLds, fit_p = npairs <= kPairLds;
  if (fit_c && t <= ncs) L.cptr[t] = p.cslot_obs_ptr[cs0 + t] - cb0;
  if (fit_b && t <= nbs) L.bptr[t] = p.bslot_pair_ptr[bs0 + t] - pb0;
  if (t < kGrp && t < o1 - o0) L.cobs[t] = p.cslot_obs[cb0 + t];
  if (fit_p)
    for (int q = t; q < npairs; q += kLinWG) L.pairs[q] = p.bslot_pairs[pb0 + q];
  double r[2], J[2][12];
  if (has) {
    const int pt = p.obs_pt[o];
    reproject_pre<true>(p.camrec[cur] + kCamRec * p.obs_cam[o], p.pts[cur] + 3 * pt,
                        p.obs_q + 2 * o, r, J);
    clamp_rows<true>(r, J);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int i = 0; i < 9; ++i) L.jc[t][9 * a + i] = J[a][i];
#pragma unroll
      for (int c = 0; c < 3; ++c) L.w[t][3 * a + c] = J[a][9 + c];
      L.w[t][6 + a] = r[a];
      L.ru[t][a] = r[a];
    }
    L.lpt[t] = pt - p0;
  }
  __syncthreads();
  if (p.cam_fixed != nullptr) {
    // held parameters: each camera slot's mask word is loaded once and dealt to
    // the slot's observations (the slots partition the group), then every
    // observation lane drops the held columns of its camera block -- in its
    // registers (W below) and in the LDS rows the slot phase reads
    for (int sl = t; sl < ncs; sl += kLinWG) {
      const unsigned fx = p.cam_fixed[p.cslot_cam[cs0 + sl]];
      const int qe = p.cslot_obs_ptr[cs0 + sl + 1] - cb0;
      for (int q = p.cslot_obs_ptr[cs0 + sl] - cb0; q < qe; ++q) L.fx[L.cobs[q]] = fx;
    }
    __syncthreads();
    if (has) {
      const unsigned fx = L.fx[t];
      if (fx) {
        hold_cols(J, fx);
#pragma unroll
        for (int i = 0; i < 9; ++i)
          if ((fx >> i) & 1u) L.jc[t][i] = L.jc[t][9 + i] = 0.0;
      }
    }
  }
  if (ROBUST && p.loss != 0) {
    // robust loss: r and all 12 columns scaled by sqrt(w), in the registers (W
    // below) and in the LDS rows the point and slot phases read
    if (has) {
      L.rho[t] = robust_weight<12>(r, J[0], J[1], p.loss, p.loss_scale);
#pragma unroll
      for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int i = 0; i < 9; ++i) L.jc[t][9 * a + i] = J[a][i];
#pragma unroll
        for (int c = 0; c < 3; ++c) L.w[t][3 * a + c] = J[a][9 + c];
        L.w[t][6 + a] = r[a];
        L.ru[t][a] = r[a];
      }
    }
    __syncthreads();
  }
  const double lam = p.state[SLAM_BA_ST_LAMBDA];
  if (t < p1 - p0) {
    const int pt = p0 + t;
    PtSchur ps;
    for (int k = p.pt_ptr[pt] - o0; k < p.pt_ptr[pt + 1] - o0; ++k) {
#pragma unroll
      for (int a = 0; a < 2; ++a) ps.acc(L.w[k][3 * a], L.w[k][3 * a + 1], L.w[k][3 * a + 2], L.w[k][6 + a]);
    }
    ps.solve(lam);
#pragma unroll
    for (int k = 0; k < 3; ++k) L.pt[t][k] = ps.e[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) L.pt[t][3 + k] = ps.iv[k];
  }
  __syncthreads();
  if (has) {
    const double* e = L.pt[L.lpt[t]];
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) L.w[t][3 * i + c] = J[0][i] * J[0][9 + c] + J[1][i] * J[1][9 + c];
    L.ru[t][2] = J[0][9] * e[0] + J[0][10] * e[1] + J[0][11] * e[2];
    L.ru[t][3] = J[1][9] * e[0] + J[1][10] * e[1] + J[1][11] * e[2];
  }
  __syncthreads();
  // the group's slot lists (staged in LDS at kernel start: see below)
  // slot phase: LDS-staged lists when they fit (always at C3), else from memory
  // (two inlined copies, so every list access is a plain ds_read or global load)
  if (fit_c && fit_b && fit_p)
    lin_slots<ROBUST>(p, L, cs0, ncs, bs0, nbs, L.cptr, 0, L.bptr, 0, L.pairs);
  else
    lin_slots<ROBUST>(p, L, cs0, ncs, bs0, nbs, p.cslot_obs_ptr + cs0, cb0, p.bslot_pair_ptr + bs0, pb0,
                      p.bslot_pairs + pb0);
}

// ---------------------------------------------------------------- camera-union linearisation
// lin_mode 1 (planner ba.plan_mfma): a workgroup owns a supergroup -- a run of
// chunks (<= kMObs observations, <= kMPts whole points each) whose points
// together see m <= kMCams cameras -- and forms its whole share of the reduced
// camera system as ONE dense (9m x 9m) matrix, on the f64 matrix cores
// (v_mfma_f64_16x16x4_f64):
//   Schur part  T = sum_p Y_p W_p^T: W_p is the point's 9m x 3 column of camera
//               blocks (W~_{p,a} = sum of Jc_o^T Jp_o over its observations by
//               camera a; zero for cameras that do not see p), Y_p = W_p V*_p^-1;
//               one MFMA per point and upper 16x16 tile of T (K = the point's
//               3 coordinates, padded to 4);
//   camera part Z_a = sum over the observation rows of camera a of z^T z with
//               z = [Jc row (9) | r | u | 0]: one 16x16 tile per camera holding
//               U_a = Jc^T Jc, Jc^T r, Jc^T u, diag U and |r|^2 (K = 2 rows of
//               2 observations per MFMA);
// accumulated in registers across the supergroup's chunks and written once:
// per camera a one cpart row (U_a - T_aa, Jc^T r, Jc^T u, diag U, |r|^2), per
// co-observed camera pair a < b one bpart row (T_ab) -- the rows k_assemble
// sums.  Per point: V, g, V*, V*^-1, e (PtSchur, as k_linearize; LDS only).
constexpr int kMObs = 120, kMPts = 16, kMCams = 7, kMRows = 64;
constexpr int kMWG = 256;
constexpr int kFoldWG = 256;   // lanes that sum in fold_rows_sum: fixes the order of the folded sums
constexpr int kSgMeta = 24;  // sg_meta record: ch0 ch1 cs0 m bs0 nb p0 p1 o0 o1 cams[8] pad
constexpr int kNoObs = 255;  // MLds::kfirst: the camera does not see the point
constexpr int kMObsS = kMObs + 1;  // odd stride: element-major arrays read across lanes without conflicts
struct alignas(16) MLds {
  // the small arrays first: their addresses fit the 16-bit offset field of an
  // LDS instruction, so no register has to hold one across the chunk loop
  double vi[kMPts][6];           // V*^-1 (i00 i01 i02 i11 i12 i22)
  double e[kMPts][3];
  double cam[kMCams][kCamRec];   // the supergroup's camera records (live parameters)
  double X[kMPts][3];            // the chunk's points
  double zero;                   // operand of padded MFMA lanes
  int optr[kMPts + 1];           // chunk-local observation range of each point
  int lpt[kMObs];                // chunk-local point of each observation
  int la[kMObs];                 // supergroup-local camera of each observation
  int cobs[kMObs];               // chunk-local observations sorted by camera
  int cptr[8];                   // their per-camera runs
  uint8_t kfirst[kMPts][8];      // first observation of (point, camera slot) in the chunk, kNoObs: none
  unsigned fx[kMCams];           // held-parameter mask word of each camera (cam_fixed only)
  int crow[kMCams];              // cpart row of each camera slot
  int bab[kMCams * (kMCams - 1) / 2], brow[kMCams * (kMCams - 1) / 2];  // block slots
  // per-observation values stored element-major ([value][obs], stride 121):
  // lanes taking consecutive observations touch consecutive doubles, and the
  // 16 lanes of an MFMA operand group (one observation, 16 values) stride by
  // an odd number of doubles (was [obs][18]: 3 LDS conflict cycles per access)
  alignas(8) double jc[18][kMObsS];  // Jc rows (2 x 9)
  double jp[6][kMObsS];          // Jp rows (2 x 3)
  double ru[4][kMObsS];          // r0 r1 u0 u1
  alignas(16) double yt[kMPts][3][kMRows];  // Y_p, [point][k][row]: the MFMA A operand
  double wt[kMPts][3][kMRows];   // W_p, [point][k][row]: the MFMA B operand
};
static_assert(sizeof(MLds) <= 80 * 1024, "k_lin_mfma: two workgroups per CU");
static_assert(offsetof(MLds, ru) == offsetof(MLds, jp) + 6 * kMObsS * sizeof(double),
              "k_lin_mfma: (B) reads Jp and r as the rows of one array");
static_assert(kMObs <= kNoObs && kMCams <= 8 && kMPts * 8 <= kMWG, "k_lin_mfma: kfirst");
static_assert(16 * kMPts <= kMWG && 2 * kMCams <= 16, "k_lin_mfma: 16 lanes per point in (B), (C)");
static_assert(kMWG == 256 && kMCams <= 7 && kMRows == 64, "k_lin_mfma: the deal of (D) covers 4 waves, 10 tiles and 7 cameras");
static_assert(9 * kMCams <= kMRows, "k_lin_mfma: 9m rows in 4 tile rows");
static_assert(kMCams * kCamRec + kMCams <= kMWG, "k_lin_mfma: a lane per record entry and per mask word");
static_assert(2 * kMPts * 3 * kMRows >= kMRows * kMRows + kMCams * 256 &&
                  offsetof(MLds, wt) == offsetof(MLds, yt) + sizeof(MLds::yt),
              "staging aliases yt/wt");

// -DSLAM_LINM_PROFILE: shader cycles per phase, summed over the workgroup's
// chunks (first lane of wave SLAM_LINM_WAVE, s_memtime): 1 staging (incl. the
// wait for the prefetched loads), 2 projections (A), 3 points (B), 4 W/Y (C), 5 MFMA + U (D),
// 6 write-out (E); slam_linm_stamps reads them (scripts/linm_prof.py).
#ifdef SLAM_LINM_PROFILE
#ifndef SLAM_LINM_WAVE
#define SLAM_LINM_WAVE 0  // the wave whose first lane takes the stamps (0..3)
#endif
#define LINM_ON (threadIdx.x == 64 * SLAM_LINM_WAVE)
__device__ unsigned long long g_linm_stamp[4096][8];
// (the sums live in LDS, not in registers of the kernel's peak)
#define LINM_DECL()                                            \
  __shared__ unsigned long long linm_acc[7];                   \
  unsigned long long linm_prev = __builtin_amdgcn_s_memtime(); \
  if (LINM_ON)                                                 \
    for (int linm_i = 0; linm_i < 7; ++linm_i) linm_acc[linm_i] = 0
#define LINM_T(i)                                                       \
  do {                                                                  \
    if (LINM_ON) {                                                      \
      const unsigned long long linm_now = __builtin_amdgcn_s_memtime(); \
      linm_acc[i] += linm_now - linm_prev;                              \
      linm_prev = linm_now;                                             \
    }                                                                   \
  } while (0)
#define LINM_END()                                                               \
  do {                                                                           \
    if (LINM_ON && blockIdx.x + 1024 * blockIdx.y < 4096)                        \
      for (int linm_i = 0; linm_i < 7; ++linm_i)                                 \
        g_linm_stamp[blockIdx.x + 1024 * blockIdx.y][linm_i] = linm_acc[linm_i]; \
  } while (0)
#else
#define LINM_DECL() (void)0
#define LINM_T(i) (void)0
#define LINM_END() (void)0
#endif

// ---------------------------------------------------------------- folded assembly
// lin_mode 1 with asm_tab (include/slam355.h): k_lin_mfma assembles the reduced
// camera system itself.  Every supergroup adds one to the counter of each block
// it wrote a partial row of, after its (sc1, write-through) row stores have
// drained; the supergroup whose add completes a block (count == need) sums that
// block's rows with sc1 loads -- its add coming last makes it the acquire for
// all the rows (MI355X_MICROARCH.md hand-off table, row 1) -- and writes the
// block into sys; blocks with no partial row here are zeroed by the build.  The
// sums run in a fixed order (rows interleaved over the parts, parts added in
// order), whichever workgroup assembles.  One dependent launch (k_assemble) and
// its wait for CU slots fewer per LM iteration.
struct AsmTab {
  const int32_t* need;
  int32_t* cnt;
  const int32_t* cam_dblk;
  const int32_t* row_blk;
  int n_empty;
  const int32_t* empty;
  __device__ explicit AsmTab(const slam_ba_problem& p) {
    const int nb = p.n_blocks;
    need = p.asm_tab;
    cnt = p.asm_tab + nb;
    cam_dblk = p.asm_tab + 2 * nb;
    row_blk = cam_dblk + p.n_cams;
    n_empty = row_blk[p.n_bslots];
    empty = row_blk + p.n_bslots + 1;
  }
};

// (a[0] + a[1]) + (a[2] + a[3]), ... : the fixed tree over N = 2^k values
template <int N>
__device__ __forceinline__ double pair_sum(const double* a) {
  if constexpr (N == 1) return a[0];
  else return pair_sum<N / 2>(a) + pair_sum<N / 2>(a + N / 2);
}

// Column sums of the n-wide rows [rb, re) of part (row stride `stride`), on the
// workgroup's first WG threads (a thread t >= WG gets k >= nparts): the lanes
// are (part k, column e) pairs; part k takes rows rb + k, rb + k + nparts, ...
// with NF loads in flight (sc1 loads when SC1: rows that other workgroups
// wrote in this launch), then the parts are added in order k = 0, 1, ...
// (deterministic).  red: LDS [nparts] rows of RS doubles (RS = 0: of n).
// Result in out[0..n).  The folded assembly (kFoldWG lanes, 4 loads, sc1) and
// k_assemble (kAsmWG lanes, 8 loads) sum in different orders: each form gives
// its own bits.
template <int WG, int NF, bool SC1, int RS>
__device__ void rows_sum(const double* __restrict__ part, int stride, int rb, int re, int n,
                         double* red, double* out) {
  const int t = threadIdx.x;
  const int nparts = WG / n, k = t / n, e = t - k * n;
  const int rs = RS ? RS : n;
  auto ld = [](const double* q) { return SC1 ? ld_sc1(q) : *q; };
  if (k < nparts) {
    double a[NF] = {};
    int r = rb + k;
    for (; r + (NF - 1) * nparts < re; r += NF * nparts) {
      double v[NF];
#pragma unroll
      for (int u = 0; u < NF; ++u) v[u] = ld(part + (size_t)(r + u * nparts) * stride + e);
#pragma unroll
      for (int u = 0; u < NF; ++u) a[u] += v[u];
    }
    for (int u = 0; r < re; r += nparts, ++u) a[u] += ld(part + (size_t)r * stride + e);
    red[k * rs + e] = pair_sum<NF>(a);
  }
  __syncthreads();
  if (t < n) {
    double v = 0.0;
    for (int q = 0; q < nparts; ++q) v += red[q * rs + t];
    out[t] = v;
  }
  __syncthreads();
}

// sys block blk (+ its camera's vectors when diagonal) from the partial rows
// (sc1 loads, 4 in flight, the parts n apart in red).  The write-out after the
// sums repeats k_assemble's statement for statement: as one shared function it
// changed both kernels' instructions (profiles/ba_dead_knobs/README.md).
template <bool ROBUST>  // the calling k_lin_mfma's: see lin_fold_assemble
__device__ void fold_block(const slam_ba_problem& p, int blk, double* scratch) {
  double* red = scratch;             // [<= 3][112]
  double* sh = scratch + 3 * kCPart;  // [112]
  double* sb = sh + kCPart;           // [81]
  const int c1 = p.blocks[2 * blk], c2 = p.blocks[2 * blk + 1];
  const int C9 = 9 * p.n_cams, t = threadIdx.x;
  double* S = p.sys;
  double* bvec = S + sys_vec_off(p.n_cams, p.n_blocks);
  double* gvec = bvec + C9;
  double* diagU = gvec + C9;
  double* costc = diagU + C9;
  const bool diag = c1 == c2;
  const int bb = p.blk_bslot_ptr[blk], be = p.blk_bslot_ptr[blk + 1];
  if (diag)
    rows_sum<kFoldWG, 4, true, 0>(p.cpart, kCPart, p.cam_cslot_ptr[c1], p.cam_cslot_ptr[c1 + 1], 109, red, sh);
  if (be > bb) {
    rows_sum<kFoldWG, 4, true, 0>(p.bpart, 81, bb, be, 81, red, sb);
  } else if (t < 81) {
    sb[t] = 0.0;
  }
  __syncthreads();
  if (sys_packed(p.n_cams)) {
    if (t < 81) S[(size_t)blk * 81 + t] = diag ? sh[t] - (sb[t] + sb[9 * (t % 9) + t / 9]) : -sb[t];
  } else if (t < 81) {
    const int i = t / 9, j = t - 9 * (t / 9);
    if (diag) {
      S[(size_t)(9 * c1 + i) * C9 + 9 * c1 + j] = sh[t] - (sb[t] + sb[9 * j + i]);
    } else {
      S[(size_t)(9 * c1 + i) * C9 + 9 * c2 + j] = -sb[t];
      S[(size_t)(9 * c2 + j) * C9 + 9 * c1 + i] = -sb[t];
    }
  }
  if (diag && t < 9) {
    gvec[9 * c1 + t] = -sh[81 + t];
    bvec[9 * c1 + t] = -sh[81 + t] - sh[90 + t];
    diagU[9 * c1 + t] = sh[99 + t];
  }
  if (diag && t == 0) costc[c1] = sh[108];
  __syncthreads();
}

// a block with no partial row in this problem: zeros (and zero vectors when
// diagonal), every build -- the packed multi-rank sys is all-reduced in place
template <bool ROBUST>  // the calling k_lin_mfma's: see lin_fold_assemble
__device__ void fold_zero_block(const slam_ba_problem& p, int blk, int t0, int nt) {
  const int c1 = p.blocks[2 * blk], c2 = p.blocks[2 * blk + 1];
  const int C9 = 9 * p.n_cams;
  double* S = p.sys;
  double* bvec = S + sys_vec_off(p.n_cams, p.n_blocks);
  for (int e = t0; e < 81; e += nt) {
    const int i = e / 9, j = e - 9 * (e / 9);
    if (sys_packed(p.n_cams)) {
      S[(size_t)blk * 81 + e] = 0.0;
    } else {
      S[(size_t)(9 * c1 + i) * C9 + 9 * c2 + j] = 0.0;
      S[(size_t)(9 * c2 + j) * C9 + 9 * c1 + i] = 0.0;
    }
  }
  if (c1 == c2)
    for (int e = t0; e < 28; e += nt) {  // b, g, diag U (9 each), cost
      if (e < 27) bvec[(size_t)(e / 9) * C9 + 9 * c1 + e % 9] = 0.0;
      else bvec[3 * (size_t)C9 + c1] = 0.0;
    }
}

// ROBUST (here, in fold_block and in fold_zero_block): the calling k_lin_mfma's,
// nothing else -- each of its two instantiations gets its own copy of these
// functions (one caller each, inlined as before the kernel was a template)
// and its own `done` / `ndone` in LDS.
template <bool ROBUST>
__device__ void lin_fold_assemble(const slam_ba_problem& p, const int* cams, int m, int nb,
                                  const int* brow, double* scratch) {
  const AsmTab A(p);
  __shared__ int done[kMCams + kMCams * (kMCams - 1) / 2];
  __shared__ int ndone;
  __builtin_amdgcn_s_waitcnt(0);  // this workgroup's partial rows have left (sc1)
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int q = 0; q < m + nb; ++q) {
      const int blk = q < m ? A.cam_dblk[cams[q]] : A.row_blk[brow[q - m]];
      const int old = (int)ticket_add(reinterpret_cast<uint32_t*>(A.cnt + blk));
      if (old == A.need[blk] - 1) {
        done[n++] = blk;
        __hip_atomic_store(A.cnt + blk, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed
      }
    }
    ndone = n;
  }
  __syncthreads();
  for (int q = 0; q < ndone; ++q) fold_block<ROBUST>(p, done[q], scratch);
}

// The deal of (D)'s accumulation units -- the 10 upper 16x16 tiles of T (12
// MFMAs per full chunk each) and the <= 7 camera tiles Z_a (8 each when the
// camera sees all 16 points of a chunk) -- over the 4 waves (one per SIMD).
// Dealt by measured time, not by MFMA count: a camera tile costs about 1.3
// times a T tile (its operands come through the cobs indirection, its MFMAs
// chain on one accumulator), and the first and last camera of a supergroup
// see few points of most chunks (profiles/ba_waves/README.md).  Was
// round-robin: 3 T + 2 Z on wave 0, a zero-fed third tile on waves 2 and 3.
// A wave's tiles share a tile row I (waves 0, 1, 3) or a tile column J (wave
// 2), so the shared operand is loaded once: 16 operand loads per K-group,
// was 24.  One nibble per wave, 15: none.
//   wave          0                1                2              3
//   tiles (0,0)(0,1)(0,2)  (1,1)(1,2)(1,3)  (0,3)(2,3)(3,3)      (2,2)
//   cams         5 6               3                2            0 1 4
// A tile with I or J >= nt or a camera >= m does not exist: its wave holds
// fewer units (the tiles and the cameras of a wave are listed so that those
// that exist come first).  Accumulators: tiles in acc[0..2] and the cameras
// in acc[3..4] on waves 0..2; the tile in acc[0] and the cameras in acc[1..3]
// on wave 3.
constexpr unsigned kDealI[3] = {0x2010u, 0x2210u, 0x2310u};   // tile s: I of wave w in nibble w
constexpr unsigned kDealJ[3] = {0x2310u, 0xF321u, 0xF332u};
constexpr unsigned kDealC[3] = {0x0235u, 0x1FF6u, 0x4FFFu};

// (D), Schur part, for a wave with NTL tiles (I[s], J[s]) in u[0..NTL), which
// share I (SHJ false) or J (SHJ true):
// T += sum_p Y_p W_p^T as ONE product over the flat index kk = 3 lp + c
// (point lp, coordinate c): K-step s of an MFMA takes kk = 4 s + k
// (k = lane >> 4), so the 3 coordinates of consecutive points pack the K = 4
// steps densely -- ceil(3 npts / 4) MFMAs per tile.  Plane kk stores row r at
// (r + 16 (kk & 3)) mod 64, so the lane groups k = 0, 1 of an operand read
// fall on different LDS banks:
// A[i][k] = Y[16I + i][kk], B[k][j] = W[16J + j][kk], kk >= 3 npts -> 0.
// Operands of 4 K-steps are loaded before their MFMAs are issued.
template <int NTL, bool SHJ>
__device__ __forceinline__ void linm_schur(const MLds& L, d4 (&u)[5], int nk, const int (&I)[3],
                                           const int (&J)[3], int lane) {
  const double* Yf = &L.yt[0][0][0];
  const double* Wf = &L.wt[0][0][0];
  const int mi = lane & 15, mk = lane >> 4;
  constexpr int NA = SHJ ? NTL : 1, NB = SHJ ? 1 : NTL;
  int ra[NA], rb[NB];
#pragma unroll
  for (int s = 0; s < NA; ++s) ra[s] = (16 * I[s] + mi + 16 * mk) & (kMRows - 1);
#pragma unroll
  for (int s = 0; s < NB; ++s) rb[s] = (16 * J[s] + mi + 16 * mk) & (kMRows - 1);
  for (int k0 = 0; k0 < nk; k0 += 16) {
    double av[4][NA], bv[4][NB];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int kk = min(k0 + 4 * v + mk, 3 * kMPts - 1);
#pragma unroll
      for (int s = 0; s < NA; ++s) av[v][s] = Yf[kk * kMRows + ra[s]];
#pragma unroll
      for (int s = 0; s < NB; ++s) bv[v][s] = Wf[kk * kMRows + rb[s]];
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const bool on = k0 + 4 * v + mk < nk;
#pragma unroll
      for (int s = 0; s < NTL; ++s)
        u[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(on ? av[v][SHJ ? s : 0] : 0.0, on ? bv[v][SHJ ? 0 : s] : 0.0,
                                                    u[s], 0, 0, 0);
    }
  }
}

// (D), camera part, for a wave with NZA cameras cam[0..NZA) in u[B0..B0 + NZA):
// Z_a += z^T z over camera a's observation rows, 2 observations per MFMA:
// lane (i = lane & 15, k = lane >> 4) supplies z[row k & 1 of obs k >> 1][i]
// as both operands (A[i][k] and B[k][i] take the same value).  The wave's
// cameras advance together, 4 MFMAs each per step, operands loaded ahead;
// past a camera's last observation: zeros.
template <int B0, int NZA>
__device__ __forceinline__ void linm_cams(const MLds& L, d4 (&u)[5], const int (&cam)[3], int lane) {
  const int mi = lane & 15, mk = lane >> 4, row = mk & 1;
  int qb[NZA], qe[NZA];
  int nsteps = 0;
#pragma unroll
  for (int s = 0; s < NZA; ++s) {
    qb[s] = __builtin_amdgcn_readfirstlane(L.cptr[cam[s]]);
    qe[s] = __builtin_amdgcn_readfirstlane(L.cptr[cam[s] + 1]);
    nsteps = max(nsteps, qe[s] - qb[s]);
  }
  for (int q = 0; q < nsteps; q += 8) {
    double z[NZA][4];
    bool ok[NZA][4];
#pragma unroll
    for (int s = 0; s < NZA; ++s)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int qq = qb[s] + q + 2 * v + (mk >> 1);
        ok[s][v] = qq < qe[s];
        const int k = L.cobs[ok[s][v] ? qq : 0];
        const double* src = mi < 9 ? &L.jc[9 * row + mi][k]
                            : mi < 11 ? &L.ru[row + 2 * (mi - 9)][k] : &L.zero;
        z[s][v] = *src;
      }
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int s = 0; s < NZA; ++s) {
        const double zv = ok[s][v] ? z[s][v] : 0.0;
        u[B0 + s] = __builtin_amdgcn_mfma_f64_16x16x4f64(zv, zv, u[B0 + s], 0, 0, 0);
      }
  }
}

// ROBUST: the instantiation that can weigh observations by a robust loss,
// launched when a problem of the batch has loss != 0 (each problem then
// branches on its own loss); in the other one the loss steps are compiled
// out: the plain path runs the code it ran before the loss existed.
template <bool ROBUST>
__global__ __launch_bounds__(kMWG) void k_lin_mfma(BaBatch bat) {
  BA_PROB_X(bat);
  const int sg = bx;
  if (sg >= p.n_sgrps) return;  // batch: grid.x covers the largest problem
  LINM_DECL();
  lm_wave_priority();
  __shared__ MLds L;
  if (p.asm_tab != nullptr) {  // folded assembly: this supergroup's share of the empty blocks
    const AsmTab A(p);
    for (int q = sg; q < A.n_empty; q += p.n_sgrps) fold_zero_block<ROBUST>(p, A.empty[q], threadIdx.x, kMWG);
  }
  const int t = threadIdx.x, lane = t & 63;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
  // the supergroup record (one hop): chunk range, slot ranges, the first
  // chunk's extents, its cameras
  const int* sm = p.sg_meta + kSgMeta * sg;
  const int ch0 = sm[0], ch1 = sm[1], cs0 = sm[2], m = sm[3], bs0 = sm[4], nb = sm[5];
  const int nt = (9 * m + 15) >> 4;  // tile rows of T
  const int cur = cur_of(p.state);
  const double lam = p.state[SLAM_BA_ST_LAMBDA];
  const bool held = p.cam_fixed != nullptr;  // uniform: without a mask (A) takes no extra step
  // robust loss (uniform: the plain loss takes no extra step): (A) scales r and
  // J by sqrt(w), so the camera tile's entry (9, 9) is sum |r~|^2, not the
  // cost; each observation's first-half lane sums its delta^2 rho(z) over the
  // chunks in rcost, reduced in a fixed order in (E) and booked on the
  // supergroup's first camera row (only the sum over the rows is consumed)
  const bool robust = ROBUST && p.loss != 0;
  double rcost = 0.0;
  // the supergroup's camera records -> LDS (one load per lane)
  if (t < kMCams * kCamRec) {
    const int a = t / kCamRec, k = t - kCamRec * (t / kCamRec);
    const int c = a < m ? sm[10 + a] : -1;
    if (c >= 0) L.cam[a][k] = p.camrec[cur][(size_t)kCamRec * c + k];
  } else if (held && t - kMCams * kCamRec < m) {  // and their held-parameter words (the next lanes)
    const int a = t - kMCams * kCamRec;
    L.fx[a] = p.cam_fixed[sm[10 + a]];
  }
  if (t == 0) L.zero = 0.0;
  // output rows of this supergroup (read at the end; loaded now, off the tail)
  if (t < m) L.crow[t] = p.cslot_row[cs0 + t];
  if (t >= 64 && t - 64 < nb) {
    L.bab[t - 64] = p.bslot_ab[bs0 + t - 64];
    L.brow[t - 64] = p.bslot_row[bs0 + t - 64];
  }
  // this wave's units (the deal above): tiles (tI[s], tJ[s]), s < ntl, cameras
  // zc[s], s < nza
  int tI[3], tJ[3], zc[3];
  int ntl = 0, nza = 0;
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    tI[s] = (kDealI[s] >> (4 * wid)) & 15;
    tJ[s] = (kDealJ[s] >> (4 * wid)) & 15;
    ntl += tJ[s] < nt;
  }
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    zc[s] = (kDealC[s] >> (4 * wid)) & 15;
    nza += zc[s] < m;
  }
  d4 acc[5];
#pragma unroll
  for (int s = 0; s < 5; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
  const int mi = lane & 15, mk = lane >> 4;

  // chunk extents: the first from the record, the next loaded one chunk ahead;
  // a chunk's inputs are loaded one chunk ahead too (issued after the current
  // chunk is staged, in flight across its phases: barriers wait on LDS only)
  struct ChunkIn {
    double q0, q1, xv;
    int meta, pp, cp;
  };
  auto load_in = [&](int t, int ch, int p0, int p1, int o0, int o1) {  // t: the lane (tl in the loop)
    ChunkIn in{0.0, 0.0, 0.0, 0, 0, 0};
    const int nobs = o1 - o0, npts = p1 - p0;
    const int ko = t & 127;  // (A) splits an observation over lanes t and t + 128
    if (ko < nobs) {
      in.q0 = p.obs_q[2 * (o0 + ko)];
      in.q1 = p.obs_q[2 * (o0 + ko) + 1];
    }
    if (t < nobs) in.meta = p.obs_meta[o0 + t];
    if (t < 3 * npts) in.xv = p.pts[cur][3 * p0 + t];
    if (t >= 128 && t - 128 <= npts) in.pp = p.pt_ptr[p0 + t - 128] - o0;
    if (t < 8) in.cp = p.chk_cptr[8 * ch + t];
    return in;
  };
  int p0 = sm[6], p1 = sm[7], o0 = sm[8], o1 = sm[9];
  int np0 = 0, np1 = 0, no0 = 0, no1 = 0;
  if (ch0 + 1 < ch1) {
    np0 = p.grp_ptr[ch0 + 1];
    np1 = p.grp_ptr[ch0 + 2];
    no0 = p.chk_optr[ch0 + 1];
    no1 = p.chk_optr[ch0 + 2];
  }
  ChunkIn in = load_in(t, ch0, p0, p1, o0, o1);
  // Y/W operand planes: rows >= 9m are zero for the workgroup's whole life --
  // all planes are zeroed once here, (C) writes every row < 9m of the planes of
  // a chunk's points (zeros for the cameras that do not see a point) and never
  // a row >= 9m.  Planes of points >= npts hold what an earlier chunk left:
  // the `on` predicate of (D) is the only guard against them.  (Was: all 64
  // rows of a chunk's 3 npts planes zeroed per chunk, 49 KB of LDS stores.)
  {
    typedef double dbl2 __attribute__((ext_vector_type(2)));
    dbl2* y2 = reinterpret_cast<dbl2*>(&L.yt[0][0][0]);
    dbl2* w2 = reinterpret_cast<dbl2*>(&L.wt[0][0][0]);
    for (int i = t; i < kMPts * 3 * kMRows / 2; i += kMWG) {
      y2[i] = dbl2{0.0, 0.0};
      w2[i] = dbl2{0.0, 0.0};
    }
  }
  for (int ch = ch0; ch < ch1; ++ch) {
    const int nobs = o1 - o0, npts = p1 - p0;
    const double q0 = in.q0, q1 = in.q1;
    __syncthreads();  // the previous chunk's readers are done with L
    // the lane index as a value of this chunk: index and address math on
    // threadIdx.x that the compiler hoists out of the chunk loop stays live
    // through (A), the kernel's register peak
    int tl = t;
    asm volatile("" : "+v"(tl));
    if (tl < nobs) {
      L.lpt[tl] = in.meta & 255;
      L.la[tl] = (in.meta >> 8) & 255;
      L.cobs[tl] = in.meta >> 16;
    }
    if (tl < 3 * npts) (&L.X[0][0])[tl] = in.xv;
    if (tl >= 128 && tl - 128 <= npts) L.optr[tl - 128] = in.pp;
    if (tl < 8) L.cptr[tl] = in.cp;
    if (tl < kMPts * 8) (&L.kfirst[0][0])[tl] = kNoObs;
    __syncthreads();
    // the first observation of each (point, camera) run (obs are sorted by
    // point, then camera), for (C)
    if (tl < nobs && (tl == 0 || L.lpt[tl - 1] != L.lpt[tl] || L.la[tl - 1] != L.la[tl]))
      L.kfirst[L.lpt[tl]][L.la[tl]] = (uint8_t)tl;
    // prefetch: the next chunk's inputs and the extents of the one after
    int nnp0 = 0, nnp1 = 0, nno0 = 0, nno1 = 0;
    if (ch + 1 < ch1) {
      in = load_in(tl, ch + 1, np0, np1, no0, no1);
      if (ch + 2 < ch1) {
        nnp0 = p.grp_ptr[ch + 2];
        nnp1 = p.grp_ptr[ch + 3];
        nno0 = p.chk_optr[ch + 2];
        nno1 = p.chk_optr[ch + 3];
      }
    }
    LINM_T(1);
    // (A) per observation: residual + Jacobian (BundleAdjustment.py:317-350),
    //     split by Jacobian columns over lanes k and k + 128 (all 4 waves busy;
    //     was lanes 0..119 only)
    {
      const int k = tl & 127;
      if (k < nobs) {
        const double q[2] = {q0, q1};
        double r[2], Jh[2][6];
        if (t < 128) {
          reproject_half<0>(L.cam[L.la[k]], L.X[L.lpt[k]], q, r, Jh);
          if (held) hold_cols_half<0>(Jh, L.fx[L.la[k]]);
          if (robust) rcost += robust_weight<6>(r, Jh[0], Jh[1], p.loss, p.loss_scale);
#pragma unroll
          for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int i = 0; i < 6; ++i) L.jc[9 * a + i][k] = Jh[a][i];
            L.ru[a][k] = r[a];
          }
        } else {
          reproject_half<1>(L.cam[L.la[k]], L.X[L.lpt[k]], q, r, Jh);
          if (held) hold_cols_half<1>(Jh, L.fx[L.la[k]]);
          if (robust) robust_weight<6>(r, Jh[0], Jh[1], p.loss, p.loss_scale);
#pragma unroll
          for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int i = 0; i < 3; ++i) L.jc[9 * a + 6 + i][k] = Jh[a][i];
#pragma unroll
            for (int c = 0; c < 3; ++c) L.jp[3 * a + c][k] = Jh[a][3 + c];
          }
        }
      }
    }
    __syncthreads();
    LINM_T(2);
    // (B) per point: V, g, V* = V + lam diag(V), V*^-1 (cofactors), e = V*^-1 g.
    //     Point lp has the 16 lanes 16 lp .. 16 lp + 15 (4 points per wave):
    //     lane j < 9 sums component j of (V, g) (pt_comp: PtSchur::acc's chain
    //     for it), the nine meet on the point's first lane by DPP row shifts (a
    //     row is these 16 lanes), which solves (was: one lane per point, 16 of
    //     256, nine chains each)
    {
      tl = t;  // again: not a value that lives through (A)
      asm volatile("" : "+v"(tl));
      const int lp = tl >> 4, j = tl & 15;
      double v = 0.0;
      if (lp < npts && j < 9) v = pt_comp(&L.jp[0][0], kMObsS, L.optr[lp], L.optr[lp + 1], j);
      PtSchur ps;
      // row_shl:j -- lane i of a row takes lane i + j's value, so the row's lane 0
      // takes component j (ds_bpermute would be an LDS round trip per dword)
      auto row_lane = [](double x, auto sh) {
        constexpr int kSh = decltype(sh)::value;
        union { double d; int w[2]; } a, b;
        a.d = x;
        b.w[0] = __builtin_amdgcn_update_dpp(0, a.w[0], 0x100 + kSh, 0xF, 0xF, false);
        b.w[1] = __builtin_amdgcn_update_dpp(0, a.w[1], 0x100 + kSh, 0xF, 0xF, false);
        return b.d;
      };
      ps.V00 = v;
      ps.V01 = row_lane(v, std::integral_constant<int, 1>{});
      ps.V02 = row_lane(v, std::integral_constant<int, 2>{});
      ps.V11 = row_lane(v, std::integral_constant<int, 3>{});
      ps.V12 = row_lane(v, std::integral_constant<int, 4>{});
      ps.V22 = row_lane(v, std::integral_constant<int, 5>{});
      ps.g0 = row_lane(v, std::integral_constant<int, 6>{});
      ps.g1 = row_lane(v, std::integral_constant<int, 7>{});
      ps.g2 = row_lane(v, std::integral_constant<int, 8>{});
      if (lp < npts && j == 0) {
        ps.solve(lam);
#pragma unroll
        for (int k = 0; k < 3; ++k) L.e[lp][k] = ps.e[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) L.vi[lp][k] = ps.iv[k];
      }
    }
    __syncthreads();
    LINM_T(3);
    // (C) per (point, camera): W~_{p,a} rows (h = 0: rows 0..4, h = 1: rows
    //     5..8) summed over the run of observations of the same (point, camera)
    //     (adjacent: obs are sorted by point, then camera), in observation
    //     order, Y = W~ V*^-1, into the operand planes; per observation u_o.
    //     Items (point lp, camera slot a < m, half h), lane 16 lp + 2 a + h: the
    //     item takes the run of camera a in the point's observations (kfirst)
    //     and writes its rows of the point's planes -- the values, or +0.0 when
    //     camera a does not see the point, so every row < 9m of the chunk's
    //     planes is written here and no pass has to zero them first.
    {
      const int lp = tl >> 4, a = (tl & 15) >> 1, hh = tl & 1;
      if (lp < npts && a < m) {
        const int ke = L.optr[lp + 1];
        const int kf = L.kfirst[lp][a];  // the run of camera a in the point's observations (staging)
        const int ib = hh ? 5 : 0, ie = hh ? 9 : 5;
        const bool seen = kf != kNoObs;
        double W[5][3];
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
          for (int c = 0; c < 3; ++c) W[i][c] = 0.0;
        for (int k = kf; k < ke && L.la[k] == a; ++k) {
#pragma unroll
          for (int i = 0; i < 5; ++i) {
            if (ib + i >= ie) break;
#pragma unroll
            for (int c = 0; c < 3; ++c)
              W[i][c] += L.jc[ib + i][k] * L.jp[c][k] + L.jc[9 + ib + i][k] * L.jp[3 + c][k];
          }
        }
        const double* vi = L.vi[lp];
        const double V[3][3] = {{vi[0], vi[1], vi[2]}, {vi[1], vi[3], vi[4]}, {vi[2], vi[4], vi[5]}};
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          if (ib + i >= ie) break;
          const int row = 9 * a + ib + i;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int pos = (row + 16 * ((3 * lp + c) & 3)) & (kMRows - 1);  // see (D)
            const double y = W[i][0] * V[0][c] + W[i][1] * V[1][c] + W[i][2] * V[2][c];
            L.wt[lp][c][pos] = W[i][c];   // +0.0 when not seen
            L.yt[lp][c][pos] = seen ? y : 0.0;
          }
        }
      }
      const int h = t >> 7, k0 = t & 127;
      if (h == 0 && k0 < nobs) {
        const double* e = L.e[L.lpt[k0]];
        L.ru[2][k0] = L.jp[0][k0] * e[0] + L.jp[1][k0] * e[1] + L.jp[2][k0] * e[2];
        L.ru[3][k0] = L.jp[3][k0] * e[0] + L.jp[4][k0] * e[1] + L.jp[5][k0] * e[2];
      }
    }
    __syncthreads();
    LINM_T(4);
    // (D) this wave's units (the deal above; linm_schur, linm_cams): no MFMA
    //     and no operand load for a unit the wave does not hold (was: a
    //     zero-fed third tile on the waves with two).  wid, ntl and nza are
    //     wave-uniform, so each wave runs one straight-line variant.
    {
      const int nk = 3 * npts;
      int ld = lane;  // a value of this chunk, as tl: the operand addresses do not live through (A)
      asm volatile("" : "+v"(ld));
      if (wid == 2) {
        if (ntl == 3) linm_schur<3, true>(L, acc, nk, tI, tJ, ld);
      } else if (ntl == 3) {
        linm_schur<3, false>(L, acc, nk, tI, tJ, ld);
      } else if (ntl == 2) {
        linm_schur<2, false>(L, acc, nk, tI, tJ, ld);
      } else if (ntl == 1) {
        linm_schur<1, false>(L, acc, nk, tI, tJ, ld);
      }
      if (wid == 3) {
        if (nza == 3) linm_cams<1, 3>(L, acc, zc, ld);
        else if (nza == 2) linm_cams<1, 2>(L, acc, zc, ld);
        else if (nza == 1) linm_cams<1, 1>(L, acc, zc, ld);
      } else if (nza == 2) {
        linm_cams<3, 2>(L, acc, zc, ld);
      } else if (nza == 1) {
        linm_cams<3, 1>(L, acc, zc, ld);
      }
    }
    p0 = np0; p1 = np1; o0 = no0; o1 = no1;
    np0 = nnp0; np1 = nnp1; no0 = nno0; no1 = nno1;
    LINM_T(5);
  }
  // (E) T and the Z_a tiles -> LDS staging (aliases the operand planes), then
  //     the partial rows
  double* rsum = &L.e[0][0];  // robust: the waves' delta^2 rho sums ((C) of the last chunk is done with e)
  if (robust) {
    for (int off = 32; off > 0; off >>= 1) rcost += __shfl_down(rcost, off, 64);  // fixed tree
    if (lane == 0) rsum[wid] = rcost;  // waves 2, 3: the second-half lanes hold 0
  }
  __syncthreads();
  double* T = &L.yt[0][0][0];
  double* Z = T + kMRows * kMRows;  // [kMCams][16][16]
#pragma unroll
  for (int s = 0; s < 5; ++s) {
    const int ts = wid == 3 ? (s == 0 ? 0 : 3) : s;   // tile slot (3: none) and
    const int zs = wid == 3 ? s - 1 : s - 3;          // camera slot (< 0: none) held by acc[s]
    if (ts < 3 && ts < ntl) {
      const int I = ts == 0 ? tI[0] : ts == 1 ? tI[1] : tI[2], J = ts == 0 ? tJ[0] : ts == 1 ? tJ[1] : tJ[2];
#pragma unroll
      for (int r = 0; r < 4; ++r) T[(16 * I + mk + 4 * r) * kMRows + 16 * J + mi] = acc[s][r];
    } else if (zs >= 0 && zs < nza) {
      const int a = zs == 0 ? zc[0] : zs == 1 ? zc[1] : zc[2];
#pragma unroll
      for (int r = 0; r < 4; ++r) Z[a * 256 + (mk + 4 * r) * 16 + mi] = acc[s][r];
    }
  }
  __syncthreads();
  const bool fold = p.asm_tab != nullptr;  // uniform
  // camera rows: items (a, 112-wide row entry)
  for (int q = t; q < m * 109; q += kMWG) {
    const int a = q / 109, e = q - 109 * (q / 109);
    const double* Za = Z + a * 256;
    double v;
    if (e < 81) {
      const int i = e / 9, j = e - 9 * (e / 9);
      const int row = 9 * a + i, col = 9 * a + j;  // T is symmetric; upper tiles were formed
      const double tv = (row >> 4) <= (col >> 4) ? T[row * kMRows + col] : T[col * kMRows + row];
      v = Za[i * 16 + j] - tv;
    } else if (e < 90) {
      v = Za[(e - 81) * 16 + 9];   // Jc^T r
    } else if (e < 99) {
      v = Za[(e - 90) * 16 + 10];  // Jc^T u
    } else if (e < 108) {
      v = Za[(e - 99) * 17];       // diag U
    } else {
      v = Za[9 * 16 + 9];          // |r|^2
      if (robust) v = a == 0 ? rsum[0] + rsum[1] : 0.0;  // sum delta^2 rho(z), on the first row
    }
    // written through (sc1) only for the folded assembly (other CUs read them in
    // this launch); plain stores keep the lines in L2 for k_assemble
    double* cp = p.cpart + (size_t)L.crow[a] * kCPart + e;
    if (fold) st_sc1(cp, v);
    else *cp = v;
  }
  for (int q = t; q < 81 * nb; q += kMWG) {
    const int pr = q / 81, e = q - 81 * (q / 81);
    const int ab = L.bab[pr], a = ab & 255, b = ab >> 8;
    const int i = e / 9, j = e - 9 * (e / 9);
    const double v = T[(9 * a + i) * kMRows + 9 * b + j];
    double* bp = p.bpart + (size_t)L.brow[pr] * 81 + e;
    if (fold) st_sc1(bp, v);
    else *bp = v;
  }
  LINM_T(6);
  if (p.asm_tab != nullptr) lin_fold_assemble<ROBUST>(p, sm + 10, m, nb, L.brow, &L.jc[0][0]);
  LINM_END();
}

#ifndef SLAM_ASM_WG
#define SLAM_ASM_WG 1024  // k_assemble workgroup (>= 128: one lane per element of a 109-double row)
#endif
constexpr int kAsmWG = SLAM_ASM_WG;
static_assert(kAsmWG >= 128 && kAsmWG % 64 == 0, "SLAM_ASM_WG");

// One workgroup per upper camera-pair block (c1 <= c2), ALL C(C+1)/2 of them.
// The slot partials of a camera / block are contiguous rows (the planner's
// camera- / block-major row order), summed in group order (deterministic):
//   diagonal block c:  S = sum (U - Y W^T) over the camera rows of c, minus
//                      B + B^T for the block rows of (c, c) (a point observed
//                      twice by c); b = -Jc^T r - Jc^T u, g = -Jc^T r, diag U, cost;
//   block c1 < c2:     S = -sum Y W^T (and its transpose) over the block rows.
// Dense layout: blocks without common points are written as zeros, so sys
// needs no separate clearing.  Packed layout: each listed block is written
// once, full 9x9, at sys + 81 * blk.
__global__ __launch_bounds__(kAsmWG) void k_assemble(BaBatch bat) {
  BA_PROB_X(bat);
  if (bx >= (p.asm_act != nullptr ? p.n_asm_act : p.n_blocks)) return;
  lm_wave_priority();
  __shared__ double red[kAsmWG / 81][kCPart];
  __shared__ double sh[kCPart];
  __shared__ double sb[81];
  const int blk = p.asm_act != nullptr ? p.asm_act[bx] : bx;
  if (p.asm_act != nullptr) {
    // this workgroup's share of the zeros of the unlisted blocks and of the
    // vector entries of the cameras without rows (what the assembly writes for
    // them: S -0.0, b and g -0.0, diag U and cost +0.0), beside the listed
    // blocks that the workgroups write (disjoint addresses, no ordering needed)
    const int32_t* listed = p.asm_act + p.n_asm_act;  // [n_blocks] 0/1
    const int32_t* camrows = listed + p.n_blocks;      // [n_cams] 0/1
    const size_t ns = (size_t)p.n_blocks * 81, c9 = 9 * (size_t)p.n_cams, nv = ns + 3 * c9 + p.n_cams;
    for (size_t i = (size_t)bx * kAsmWG + threadIdx.x; i < nv; i += (size_t)p.n_asm_act * kAsmWG) {
      if (i < ns) {
        if (!listed[i / 81]) p.sys[i] = -0.0;
      } else {
        const size_t j = i - ns;
        const int cam = j < 3 * c9 ? (int)((j % c9) / 9) : (int)(j - 3 * c9);
        if (!camrows[cam]) p.sys[i] = j < 2 * c9 ? -0.0 : 0.0;
      }
    }
  }
  const int c1 = p.blocks[2 * blk], c2 = p.blocks[2 * blk + 1];
  const int C9 = 9 * p.n_cams;
  double* S = p.sys;
  double* bvec = S + sys_vec_off(p.n_cams, p.n_blocks);
  double* gvec = bvec + C9;
  double* diagU = gvec + C9;
  double* costc = diagU + C9;
  const int t = threadIdx.x;
  const bool diag = c1 == c2;
  const int bb = p.blk_bslot_ptr[blk], be = p.blk_bslot_ptr[blk + 1];
  if (!diag && be == bb) {
    // a block without partial rows (most listed blocks of a landmark shard:
    // the global block list, this rank's points): its zeros (-sum of nothing,
    // bit for bit what the sum path writes) without the row sums' barriers
    if (t < 81) {
      if (sys_packed(p.n_cams)) {
        S[(size_t)blk * 81 + t] = -0.0;
      } else {
        const int i = t / 9, j = t - 9 * (t / 9);
        S[(size_t)(9 * c1 + i) * C9 + 9 * c2 + j] = -0.0;
        S[(size_t)(9 * c2 + j) * C9 + 9 * c1 + i] = -0.0;
      }
    }
    return;
  }
  // plain loads, 8 in flight, the parts in rows of red
  if (diag)
    rows_sum<kAsmWG, 8, false, kCPart>(p.cpart, kCPart, p.cam_cslot_ptr[c1], p.cam_cslot_ptr[c1 + 1], 109,
                                       &red[0][0], sh);
  if (!diag || be > bb) {
    rows_sum<kAsmWG, 8, false, kCPart>(p.bpart, 81, bb, be, 81, &red[0][0], sb);
  } else if (t < 81) {
    sb[t] = 0.0;
  }
  __syncthreads();
  // the block write-out (the same statements in fold_block: see there)
  if (sys_packed(p.n_cams)) {
    if (t < 81) S[(size_t)blk * 81 + t] = diag ? sh[t] - (sb[t] + sb[9 * (t % 9) + t / 9]) : -sb[t];
  } else if (t < 81) {
    const int i = t / 9, j = t - 9 * (t / 9);
    if (diag) {
      S[(size_t)(9 * c1 + i) * C9 + 9 * c1 + j] = sh[t] - (sb[t] + sb[9 * j + i]);
    } else {
      S[(size_t)(9 * c1 + i) * C9 + 9 * c2 + j] = -sb[t];
      S[(size_t)(9 * c2 + j) * C9 + 9 * c1 + i] = -sb[t];
    }
  }
  if (diag && t < 9) {
    gvec[9 * c1 + t] = -sh[81 + t];
    bvec[9 * c1 + t] = -sh[81 + t] - sh[90 + t];
    diagU[9 * c1 + t] = sh[99 + t];
  }
  if (diag && t == 0) costc[c1] = sh[108];
}

__device__ void lm_decide(double* __restrict__ state, const double* __restrict__ small);

// Back substitution + trial cost, one workgroup per point group:
//   per observation: Jacobian at the live parameters (the one the lineariser
//     used), Jp and r -> LDS, w_o = W_o^T dc = Jp^T (Jc dc_cam(o))   (-> LDS)
//   per point: V, g, diag, V*^-1, e re-derived in the lineariser's operation
//     order (PtSchur: bit-identical to what it used -- no per-point record
//     written by the lineariser and read back here), dp = e - sum_o V*^-1 w_o,
//     trial point x + dp, predicted-reduction term
//   per observation: trial residual at (cams[next], trial point)   (-> |r|^2)
// Workgroup partial sums go to part[g] (cost) and part[G + g] (pred) as sc1
// stores; the last workgroup to finish (agent-scope ticket) sums them in a
// fixed order into small[0..1] and, when DECIDE (single rank), applies the LM
// decision.
template <bool DECIDE, bool ROBUST>  // ROBUST as k_lin_mfma
__global__ __launch_bounds__(kGrp) void k_back_trial(BaBatch bat) {
  BA_PROB_X(bat);
  const int g = bx, G = p.n_grps;
  if (g >= G) return;  // batch: grid.x covers the largest problem (not in the ticket count)
  double* __restrict__ part = p.red_part;
  lm_wave_priority();
  __shared__ double sjp[6][kGrp + 1], sr[2][kGrp + 1], sw[3][kGrp + 1];  // [value][obs]
  __shared__ double snp[kGrp][3];
  __shared__ double red[kGrp / 64];
  __shared__ int last;
  // group extents in one hop (chk_optr = pt_ptr[grp_ptr])
  const int p0 = p.grp_ptr[g], p1 = p.grp_ptr[g + 1];
  const int o0 = p.chk_optr[g], o1 = p.chk_optr[g + 1];
  const int t = threadIdx.x;
  const int o = o0 + t;
  const bool has = o < o1;
  const int cur = cur_of(p.state);
  const bool fail = p.state[SLAM_BA_ST_CHOL_FAIL] != 0.0;
  // the point lanes' inputs, loaded before the observation phase
  const bool ptl = t < p1 - p0;
  double xv[3];
  int kb = 0, ke = 0;
  if (ptl) {
#pragma unroll
    for (int k = 0; k < 3; ++k) xv[k] = p.pts[cur][3 * (p0 + t) + k];
    kb = p.pt_ptr[p0 + t] - o0;
    ke = p.pt_ptr[p0 + t + 1] - o0;
  }
  if (has) {
    double r[2], J[2][12];
    const int pt = p.obs_pt[o];
    reproject_pre<true>(p.camrec[cur] + kCamRec * p.obs_cam[o], p.pts[cur] + 3 * pt,
                        p.obs_q + 2 * o, r, J);
    clamp_rows<true>(r, J);
    // the lineariser's weights (a held column only ever multiplies its zero
    // step below, so hold_cols is not repeated here)
    if (ROBUST && p.loss != 0) robust_weight<12>(r, J[0], J[1], p.loss, p.loss_scale);
    const double* dc = p.delta_c + 9 * p.obs_cam[o];
    double w0 = 0.0, w1 = 0.0, w2 = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const double c = dc[i];
      w0 += (J[0][i] * J[0][9] + J[1][i] * J[1][9]) * c;
      w1 += (J[0][i] * J[0][10] + J[1][i] * J[1][10]) * c;
      w2 += (J[0][i] * J[0][11] + J[1][i] * J[1][11]) * c;
    }
    sw[0][t] = w0;
    sw[1][t] = w1;
    sw[2][t] = w2;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int c = 0; c < 3; ++c) sjp[3 * a + c][t] = J[a][9 + c];
      sr[a][t] = r[a];
    }
  }
  __syncthreads();
  double pred = 0.0;
  if (ptl) {
    const int pt = p0 + t;
    const double lam = p.state[SLAM_BA_ST_LAMBDA];
    PtSchur ps;
    for (int k = kb; k < ke; ++k) {
#pragma unroll
      for (int a = 0; a < 2; ++a) ps.acc(sjp[3 * a][k], sjp[3 * a + 1][k], sjp[3 * a + 2][k], sr[a][k]);
    }
    ps.solve(lam);
    const double* iv = ps.iv;
    double d0 = ps.e[0], d1 = ps.e[1], d2 = ps.e[2];
    for (int k = kb; k < ke; ++k) {
      const double w0 = sw[0][k], w1 = sw[1][k], w2 = sw[2][k];
      d0 -= iv[0] * w0 + iv[1] * w1 + iv[2] * w2;
      d1 -= iv[1] * w0 + iv[3] * w1 + iv[4] * w2;
      d2 -= iv[2] * w0 + iv[4] * w1 + iv[5] * w2;
    }
    const double* x = xv;
    double* xn = p.pts[1 - cur] + 3 * pt;
    snp[t][0] = xn[0] = x[0] + d0;
    snp[t][1] = xn[1] = x[1] + d1;
    snp[t][2] = xn[2] = x[2] + d2;
    pred = d0 * (lam * ps.d[0] * d0 + ps.g0) + d1 * (lam * ps.d[1] * d1 + ps.g1) +
           d2 * (lam * ps.d[2] * d2 + ps.g2);
    if (fail) pred = 0.0;
  }
  __syncthreads();
  double v = 0.0;
  if (has) {
    double r[2], J[2][12];
    reproject_pre<false>(p.camrec[1 - cur] + kCamRec * p.obs_cam[o], snp[p.obs_pt[o] - p0],
                         p.obs_q + 2 * o, r, J);
    clamp_rows<false>(r, J);
    if (ROBUST && p.loss != 0) v = robust_weight<0>(r, nullptr, nullptr, p.loss, p.loss_scale);  // delta^2 rho(z)
    else v = r[0] * r[0] + r[1] * r[1];
  }
  v = block_sum(v, red);
  pred = block_sum(pred, red);
  if (t == 0) {
    st_sc1(part + g, v);
    st_sc1(part + G + g, pred);
    __builtin_amdgcn_s_waitcnt(0);  // drained before the ticket
    last = ticket_add(p.ticket) == (unsigned)(G - 1);
  }
  __syncthreads();
  if (!last) return;
  double a = 0.0, b = 0.0;
  for (int i = t; i < G; i += kGrp) {
    a += ld_sc1(part + i);
    b += ld_sc1(part + G + i);
  }
  a = block_sum(a, red);
  b = block_sum(b, red);
  if (t == 0) {
    p.small[0] = a;
    p.small[1] = b;
    ticket_reset(p.ticket);  // re-arm for the next launch
    if (DECIDE) lm_decide(p.state, p.small);
  }
}

__global__ void k_decide(BaBatch bat) {
  BA_PROB(bat);
  if (threadIdx.x == 0) lm_decide(p.state, p.small);
}

__device__ void lm_decide(double* __restrict__ state, const double* __restrict__ small) {
  const double cost = state[SLAM_BA_ST_COST];
  const double cost_new = 0.5 * small[0];
  const double pred = state[SLAM_BA_ST_PRED_CAM] + 0.5 * small[1];
  const bool fail = state[SLAM_BA_ST_CHOL_FAIL] != 0.0;
  const double rho = (!fail && pred > 0.0) ? (cost - cost_new) / pred : -1.0;
  double lam = state[SLAM_BA_ST_LAMBDA], nu = state[SLAM_BA_ST_NU];
  const bool acc = rho > 0.0 && isfinite(cost_new);
  if (acc) {
    const double t = 2.0 * rho - 1.0;
    lam *= fmax(1.0 / 3.0, 1.0 - t * t * t);
    lam = fmin(fmax(lam, kLamMin), kLamMax);
    nu = 2.0;
    state[SLAM_BA_ST_CUR] = state[SLAM_BA_ST_CUR] != 0.0 ? 0.0 : 1.0;
    state[SLAM_BA_ST_COST] = cost_new;
    state[SLAM_BA_ST_NACCEPT] += 1.0;
  } else {
    lam = fmin(lam * nu, kLamMax);
    nu *= 2.0;
  }
  state[SLAM_BA_ST_LAMBDA] = lam;
  state[SLAM_BA_ST_NU] = nu;
  state[SLAM_BA_ST_COST_NEW] = cost_new;
  state[SLAM_BA_ST_PRED] = pred;
  state[SLAM_BA_ST_RHO] = rho;
  state[SLAM_BA_ST_ACCEPTED] = acc ? 1.0 : 0.0;
  state[SLAM_BA_ST_ITERS] += 1.0;
}

__global__ void k_reset(BaBatch bat, double lam0) {
  BA_PROB(bat);
  const int t = threadIdx.x;
  double* state = p.state;
  if (t < SLAM_BA_ST_SLOTS) state[t] = 0.0;
  if (t == 0) {
    state[SLAM_BA_ST_LAMBDA] = lam0;
    state[SLAM_BA_ST_NU] = 2.0;
  }
  for (int c = t; c < p.n_cams; c += blockDim.x) cam_prep(p.cams[0] + 9 * c, p.camrec[0] + kCamRec * c);
}


int check_problem(const slam_ba_problem* p) {
  SLAM_REQUIRE(p != nullptr, "slam_ba: null problem");
  SLAM_REQUIRE(p->n_cams > 0 && p->n_pts >= 0 && p->n_obs >= 0, "slam_ba: bad sizes");
  SLAM_REQUIRE(p->loss >= 0 && p->loss <= 3,
               "slam_ba: loss %d (0 linear, 1 huber, 2 soft_l1, 3 cauchy)", p->loss);
  SLAM_REQUIRE(p->loss == 0 || (std::isfinite(p->loss_scale) && p->loss_scale > 0.0),
               "slam_ba: loss %d needs a finite loss_scale > 0, not %g", p->loss, p->loss_scale);
  SLAM_REQUIRE(p->cams[0] && p->cams[1] && p->camrec[0] && p->camrec[1] &&
                   p->cpart && p->bpart && p->grp_ptr && p->grp_cslot && p->grp_bslot &&
                   p->cslot_obs_ptr && p->bslot_pair_ptr && p->cam_cslot_ptr && p->cslot_row && p->bslot_row &&
                   p->blk_bslot_ptr && p->blocks && p->ticket && p->sys && p->state &&
                   p->small && p->red_part && p->delta_c,
               "slam_ba: null buffer");
  SLAM_REQUIRE(p->n_grps >= 1, "slam_ba: n_grps must be >= 1 (an empty group for P = 0)");
  SLAM_REQUIRE(p->lin_mode == 0 || p->lin_mode == 1, "slam_ba: lin_mode must be 0 or 1");
  SLAM_REQUIRE(p->chk_optr != nullptr, "slam_ba: chk_optr (= pt_ptr[grp_ptr]) required");
  SLAM_REQUIRE(p->lin_mode == 0 || (p->n_sgrps >= 1 && p->sg_ptr && p->sg_meta && p->obs_meta &&
                                     p->chk_cptr && p->bslot_ab),
               "slam_ba: lin_mode 1 needs n_sgrps >= 1 and the supergroup tables");
  SLAM_REQUIRE(sys_packed(p->n_cams) ? (p->n_blocks >= p->n_cams &&
                                        p->n_blocks <= p->n_cams * (p->n_cams + 1) / 2)
                                     : p->n_blocks == p->n_cams * (p->n_cams + 1) / 2,
               "slam_ba: n_blocks must list all C(C+1)/2 upper blocks (9C <= %d) or the "
               "diagonal and every block with common points (packed)", kDenseMaxN);
  SLAM_REQUIRE(!p->tl_sched == !p->tl_sched_host,
               "slam_ba: tl_sched and tl_sched_host come together");
  SLAM_REQUIRE(p->asm_act == nullptr ||
                   (sys_packed(p->n_cams) && p->asm_tab == nullptr && p->n_asm_act >= 1 &&
                    p->n_asm_act <= p->n_blocks),
               "slam_ba: asm_act (n_asm_act %d of %d blocks) needs a packed system without asm_tab",
               p->n_asm_act, p->n_blocks);
  SLAM_REQUIRE(p->tl_mode == 0 || p->tl_mode == 1, "slam_ba: tl_mode must be 0 or 1");
  SLAM_REQUIRE(!sys_packed(p->n_cams) || p->chol != nullptr,
               "slam_ba: chol workspace (slam_ba_chol_len doubles) required for 9C > %d",
               kLdsMaxN);
  SLAM_REQUIRE(!sys_packed(p->n_cams) || p->tl_sched != nullptr,
               "slam_ba: the tile schedule (tl_sched, ba.tl_schedule) is required for 9C > %d",
               kLdsMaxN);
  return SLAM_OK;
}

}  // namespace

extern "C" int slam_ba_red_slots(int n_grps) { return 2 * n_grps; }

extern "C" int slam_ba_problem_size(void) { return (int)sizeof(slam_ba_problem); }

extern "C" long long slam_ba_sys_len(int n_cams, int n_blocks) {
  const long long c9 = 9ll * n_cams;
  return sys_vec_off(n_cams, n_blocks) + 3 * c9 + n_cams;
}

extern "C" int slam_ba_residual(const double* d_cams, const double* d_pts,
                                const int32_t* d_cam_idx, const int32_t* d_pt_idx,
                                const double* d_qs, int n_obs, double* d_resid, void* stream) {
  SLAM_REQUIRE(n_obs >= 0, "slam_ba_residual: n_obs < 0");
  if (n_obs == 0) return SLAM_OK;
  SLAM_REQUIRE(d_cams && d_pts && d_cam_idx && d_pt_idx && d_qs && d_resid,
               "slam_ba_residual: null pointer");
  k_residual<<<nblk(n_obs, kBS), kBS, 0, slam::as_stream(stream)>>>(
      d_cams, d_pts, d_cam_idx, d_pt_idx, d_qs, n_obs, d_resid, nullptr);
  SLAM_LAUNCHED("k_residual");
  return SLAM_OK;
}

extern "C" int slam_ba_jacobian(const double* d_cams, const double* d_pts,
                                const int32_t* d_cam_idx, const int32_t* d_pt_idx,
                                const double* d_qs, int n_obs, double* d_resid, double* d_jac,
                                void* stream) {
  SLAM_REQUIRE(n_obs >= 0, "slam_ba_jacobian: n_obs < 0");
  if (n_obs == 0) return SLAM_OK;
  SLAM_REQUIRE(d_cams && d_pts && d_cam_idx && d_pt_idx && d_qs && d_resid && d_jac,
               "slam_ba_jacobian: null pointer");
  k_residual<<<nblk(n_obs, kBS), kBS, 0, slam::as_stream(stream)>>>(
      d_cams, d_pts, d_cam_idx, d_pt_idx, d_qs, n_obs, d_resid, d_jac);
  SLAM_LAUNCHED("k_residual(jac)");
  return SLAM_OK;
}

namespace {

// LDS floor of the one-workgroup camera solve (slam_ba_set_solve_lds_floor): a
// floor above what a co-resident ORB workgroup leaves keeps the latency-bound
// pivot chain off CUs whose SIMDs are busy with ORB waves.
static size_t g_solve_lds_floor = 0;

// slam_ba_set_fused_assembly: slam_ba_iterate_batch lets the one-workgroup
// camera solve sum the partial rows itself (k_solve_blk<true>) instead of
// launching k_assemble before it.  Same bits either way.
static int g_fused_assembly = 1;  // 0 never, 1 up to kFuseMaxRows partial rows per window, 2 always
// One workgroup sums a window's rows where k_assemble spreads them over a
// 1024-lane workgroup per block, so the fused form pays only while the rows
// are few: the tracker's windows (16 chunks per supergroup) have ~450, a
// window planned one chunk per supergroup ~6500 (profiles/ba_asm_solve/README.md).
constexpr int kFuseMaxRows = 1024;

static int launch_reset(const Launch& L, double lam0, hipStream_t s) {
  k_reset<<<dim3(1, L.n), 64, 0, s>>>(L.b, lam0);
  SLAM_LAUNCHED("k_reset");
  return SLAM_OK;
}

}  // namespace

int slam::make_launch(const slam_ba_problem* probs, int n, Launch* L) {
  SLAM_REQUIRE(n >= 1 && n <= kBaMaxBatch, "slam_ba: batch of %d problems (1..%d)", n, kBaMaxBatch);
  SLAM_REQUIRE(probs != nullptr, "slam_ba: null problem array");
  L->n = n;
  L->max_grps = L->max_blocks = L->max_sgrps = 0;
  L->mode = probs[0].lin_mode;
  L->solve_lds = 0;
  L->dense = true;
  L->robust = false;
  L->fused = false;
  for (int i = 0; i < n; ++i) {
    if (int rc = check_problem(probs + i)) return rc;
    for (int j = 0; j < i; ++j)
      SLAM_REQUIRE(probs[j].state != probs[i].state && probs[j].sys != probs[i].sys,
                   "slam_ba: problems %d and %d of a batch share buffers", j, i);
    SLAM_REQUIRE(probs[i].lin_mode == L->mode,
                 "slam_ba: problems of one batch must share lin_mode");
    L->b.p[i] = probs[i];
    L->max_grps = max(L->max_grps, probs[i].n_grps);
    L->max_sgrps = max(L->max_sgrps, probs[i].n_sgrps);
    L->max_blocks = max(L->max_blocks, probs[i].asm_act != nullptr ? probs[i].n_asm_act : probs[i].n_blocks);
    L->solve_lds = std::max(L->solve_lds, slam::solve_blk_lds(probs[i].n_cams));
    L->solve_lds = std::max(L->solve_lds, g_solve_lds_floor);
    L->dense = L->dense && !sys_packed(probs[i].n_cams);
    L->robust = L->robust || probs[i].loss != 0;
  }
  SLAM_REQUIRE(n == 1 || L->dense,
               "slam_ba: batched problems must use the one-workgroup solver (9C <= %d)", kLdsMaxN);
  return SLAM_OK;
}

int slam::launch_build(const Launch& L, hipStream_t s) {
  // every entry of sys is written by the assembly (all listed blocks), so no clearing
  bool folded = L.mode == 1;
  for (int i = 0; i < L.n; ++i) folded = folded && L.b.p[i].asm_tab != nullptr;
  if (L.mode == 1) {
    if (L.robust) k_lin_mfma<true><<<dim3(L.max_sgrps, L.n), kMWG, 0, s>>>(L.b);
    else k_lin_mfma<false><<<dim3(L.max_sgrps, L.n), kMWG, 0, s>>>(L.b);
    SLAM_LAUNCHED("k_lin_mfma");
  } else {
    if (L.robust) k_linearize<true><<<dim3(L.max_grps, L.n), kLinWG, 0, s>>>(L.b);
    else k_linearize<false><<<dim3(L.max_grps, L.n), kLinWG, 0, s>>>(L.b);
    SLAM_LAUNCHED("k_linearize");
  }
  if (!folded && !L.fused) {  // k_lin_mfma skips the fold of a problem without asm_tab
    k_assemble<<<dim3(L.max_blocks, L.n), kAsmWG, 0, s>>>(L.b);
    SLAM_LAUNCHED("k_assemble");
  }
  return SLAM_OK;
}

namespace {

static int launch_solve(const Launch& L, bool fuse_decide, hipStream_t s) {
  if (int rc = L.dense ? slam::launch_solve_blk(L, s) : slam::launch_solve_tiled(L.b.p[0], s)) return rc;
  if (L.robust) {
    if (fuse_decide) k_back_trial<true, true><<<dim3(L.max_grps, L.n), kGrp, 0, s>>>(L.b);
    else k_back_trial<false, true><<<dim3(L.max_grps, L.n), kGrp, 0, s>>>(L.b);
  } else if (fuse_decide) {
    k_back_trial<true, false><<<dim3(L.max_grps, L.n), kGrp, 0, s>>>(L.b);
  } else {
    k_back_trial<false, false><<<dim3(L.max_grps, L.n), kGrp, 0, s>>>(L.b);
  }
  SLAM_LAUNCHED("k_back_trial");
  return SLAM_OK;
}

}  // namespace

extern "C" int slam_ba_set_solve_lds_floor(int bytes) {
  SLAM_REQUIRE(bytes >= 0 && bytes <= 160 * 1024, "slam_ba_set_solve_lds_floor: %d B", bytes);
  g_solve_lds_floor = (size_t)bytes;
  return SLAM_OK;
}

extern "C" int slam_ba_set_fused_assembly(int on) {
  SLAM_REQUIRE(on >= 0 && on <= 2, "slam_ba_set_fused_assembly: %d (0, 1 or 2)", on);
  g_fused_assembly = on;
  return SLAM_OK;
}

extern "C" int slam_ba_reset(const slam_ba_problem* prob, double lambda0, void* stream) {
  return slam_ba_reset_batch(prob, 1, lambda0, stream);
}

extern "C" int slam_ba_reset_batch(const slam_ba_problem* probs, int n_probs, double lambda0,
                                   void* stream) {
  SLAM_REQUIRE(n_probs >= 0, "slam_ba_reset_batch: n_probs < 0");
  SLAM_REQUIRE(n_probs == 0 || probs != nullptr, "slam_ba_reset_batch: null problem array");
  for (int i0 = 0; i0 < n_probs; i0 += kBaMaxBatch) {
    Launch L;
    const int n = min(kBaMaxBatch, n_probs - i0);
    for (int i = 0; i < n; ++i)
      if (int rc = check_problem(probs + i0 + i)) return rc;
    L.n = n;
    for (int i = 0; i < n; ++i) L.b.p[i] = probs[i0 + i];
    if (int rc = launch_reset(L, lambda0, slam::as_stream(stream))) return rc;
  }
  return SLAM_OK;
}

extern "C" int slam_ba_build_system(const slam_ba_problem* prob, void* stream) {
  Launch L;
  if (int rc = make_launch(prob, 1, &L)) return rc;
  return launch_build(L, slam::as_stream(stream));
}

extern "C" int slam_ba_solve_step(const slam_ba_problem* prob, void* stream) {
  Launch L;
  if (int rc = make_launch(prob, 1, &L)) return rc;
  return launch_solve(L, false, slam::as_stream(stream));
}

extern "C" int slam_ba_decide(const slam_ba_problem* prob, void* stream) {
  Launch L;
  if (int rc = make_launch(prob, 1, &L)) return rc;
  k_decide<<<dim3(1, 1), 64, 0, slam::as_stream(stream)>>>(L.b);
  SLAM_LAUNCHED("k_decide");
  return SLAM_OK;
}

extern "C" int slam_ba_iterate(const slam_ba_problem* prob, int n_iter, void* stream) {
  return slam_ba_iterate_batch(prob, 1, n_iter, stream);
}

extern "C" int slam_ba_iterate_batch(const slam_ba_problem* probs, int n_probs, int n_iter,
                                     void* stream) {
  SLAM_REQUIRE(n_probs >= 0 && n_iter >= 0, "slam_ba_iterate_batch: negative count");
  SLAM_REQUIRE(n_probs == 0 || probs != nullptr, "slam_ba_iterate_batch: null problem array");
  hipStream_t s = slam::as_stream(stream);
  // dense problems in chunks of kBaMaxBatch share launches; a packed (tiled
  // solver) problem iterates on its own
  int i0 = 0;
  while (i0 < n_probs) {
    int n = 0;
    while (n < kBaMaxBatch && i0 + n < n_probs && (n == 0 || !sys_packed(probs[i0 + n].n_cams)) &&
           !(n > 0 && sys_packed(probs[i0].n_cams)))
      ++n;
    Launch L;
    if (int rc = make_launch(probs + i0, n, &L)) return rc;
    // the dense launch without folded assembly (asm_tab) or block shards
    // (asm_act): the solve's workgroup assembles
    L.fused = g_fused_assembly != 0 && L.dense;
    for (int i = 0; i < n; ++i) {
      const slam_ba_problem& q = probs[i0 + i];
      L.fused = L.fused && q.asm_tab == nullptr && q.asm_act == nullptr &&
                (g_fused_assembly == 2 || q.n_cslots + q.n_bslots <= kFuseMaxRows);
    }
    for (int it = 0; it < n_iter; ++it) {
      if (int rc = launch_build(L, s)) return rc;
      if (int rc = launch_solve(L, true, s)) return rc;  // decide fused into the last group
    }
    i0 += n;
  }
  return SLAM_OK;
}

#ifdef SLAM_LINM_PROFILE
extern "C" int slam_linm_stamps(unsigned long long* out, int n) {
  SLAM_HIP(hipDeviceSynchronize());
  SLAM_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_linm_stamp), (size_t)n * 8 * sizeof(unsigned long long)));
  return SLAM_OK;
}
#endif
