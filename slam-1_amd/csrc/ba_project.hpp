// The BAL projection.  The per-camera half (cam_prep): k_reset and the solve
// epilogue prepare the camera records with it.  The per-observation half
// (reproject*, the clamp, held columns, the robust weight): the linearisers and
// the back substitution of ba.hip and the landmark covariance of ba_cov.hip.
#pragma once

#include "ba_layout.hpp"
#include "robust_loss.hpp"

namespace {

// Per-camera part of the projection: everything that depends on the rotation
// vector only (theta, v, cos, sin, R and the Jacobian's A matrix), computed
// once per camera by cam_prep and stored as a 32-double record; the per-
// observation part (reproject_pre) then does no sqrt/sin/cos/division by theta.
// Both halves keep the operation order of the single-function form, so
// results are bit-identical to computing everything per observation.
__device__ __forceinline__ void cam_prep(const double* __restrict__ cam, double* __restrict__ o) {
  const double w0 = cam[0], w1 = cam[1], w2 = cam[2];
  const double th = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
  double v0 = 0.0, v1 = 0.0, v2 = 0.0;  // nan_to_num(w / 0) == 0  (:292-293)
  if (th > 0.0) {
    v0 = w0 / th;
    v1 = w1 / th;
    v2 = w2 / th;
  }
  const double c = cos(th), s = sin(th);
  const double omc = 1.0 - c;
  // R = c I + s [v]x + (1-c) v v^T
  double R[3][3];
  R[0][0] = c + omc * v0 * v0; R[0][1] = -s * v2 + omc * v0 * v1; R[0][2] = s * v1 + omc * v0 * v2;
  R[1][0] = s * v2 + omc * v1 * v0; R[1][1] = c + omc * v1 * v1; R[1][2] = -s * v0 + omc * v1 * v2;
  R[2][0] = -s * v1 + omc * v2 * v0; R[2][1] = s * v0 + omc * v2 * v1; R[2][2] = c + omc * v2 * v2;
  // dRX/dw (Gallego & Yezzi): -R [X]x A / |w|^2 with A = w w^T + (R^T - I)[w]x
  const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
  const double W[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
  const double w[3] = {w0, w1, w2};
  double A[3][3];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) {
      double acc = w[i] * w[k];
      for (int j = 0; j < 3; ++j) acc += R[j][i] * W[j][k];
      A[i][k] = acc - W[i][k];
    }
  o[0] = c; o[1] = s; o[2] = omc;
  o[3] = v0; o[4] = v1; o[5] = v2;
  for (int i = 0; i < 9; ++i) o[6 + i] = R[i / 3][i % 3];
  for (int i = 0; i < 9; ++i) o[15 + i] = A[i / 3][i % 3];
  o[24] = th2 < 1e-24 ? 0.0 : -1.0 / th2;
  o[25] = th2 < 1e-24 ? 1.0 : 0.0;
  for (int i = 0; i < 6; ++i) o[26 + i] = cam[3 + i];
}

constexpr double kClamp = 5000.0;

// ---------------------------------------------------------------- projection
// Residual (proj - q) of BundleAdjustment.py:317-337 with the operation order
// of the numpy code, and optionally its analytic 2x12 Jacobian, from a camera
// record of cam_prep.
template <bool JAC>
__device__ __forceinline__ void reproject_pre(const double* __restrict__ cr,
                                              const double* __restrict__ X,
                                              const double* __restrict__ q, double r[2],
                                              double J[2][12]) {
  const double c = cr[0], s = cr[1], omc = cr[2];
  const double v0 = cr[3], v1 = cr[4], v2 = cr[5];
  const double X0 = X[0], X1 = X[1], X2 = X[2];
  const double dot = X0 * v0 + X1 * v1 + X2 * v2;
  const double cx0 = v1 * X2 - v2 * X1;
  const double cx1 = v2 * X0 - v0 * X2;
  const double cx2 = v0 * X1 - v1 * X0;
  const double dk = dot * omc;
  const double RX0 = c * X0 + s * cx0 + dk * v0;
  const double RX1 = c * X1 + s * cx1 + dk * v1;
  const double RX2 = c * X2 + s * cx2 + dk * v2;
  const double P0 = RX0 + cr[26], P1 = RX1 + cr[27], P2 = RX2 + cr[28];
  const double p0 = -P0 / P2, p1 = -P1 / P2;
  const double f = cr[29], k1 = cr[30], k2 = cr[31];
  const double n = p0 * p0 + p1 * p1;
  const double rad = 1.0 + k1 * n + k2 * (n * n);
  const double sc = rad * f;
  r[0] = p0 * sc - q[0];
  r[1] = p1 * sc - q[1];
  if constexpr (JAC) {
    double R[3][3], A[3][3];
    for (int i = 0; i < 9; ++i) {
      R[i / 3][i % 3] = cr[6 + i];
      A[i / 3][i % 3] = cr[15 + i];
    }
    double dR[3][3];
    if (cr[25] != 0.0) {  // |w|^2 < 1e-24: -[RX]x
      dR[0][0] = 0.0;  dR[0][1] = RX2;  dR[0][2] = -RX1;
      dR[1][0] = -RX2; dR[1][1] = 0.0;  dR[1][2] = RX0;
      dR[2][0] = RX1;  dR[2][1] = -RX0; dR[2][2] = 0.0;
    } else {
      const double Xs[3][3] = {{0.0, -X2, X1}, {X2, 0.0, -X0}, {-X1, X0, 0.0}};
      double B[3][3];
      for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k)
          B[i][k] = Xs[i][0] * A[0][k] + Xs[i][1] * A[1][k] + Xs[i][2] * A[2][k];
      const double inv = cr[24];
      for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k)
          dR[i][k] = (R[i][0] * B[0][k] + R[i][1] * B[1][k] + R[i][2] * B[2][k]) * inv;
    }
    // dp/dP
    const double iz = 1.0 / P2;
    const double dpP[2][3] = {{-iz, 0.0, P0 * iz * iz}, {0.0, -iz, P1 * iz * iz}};
    // dproj/dp = sc I + 2 f (k1 + 2 k2 n) p p^T
    const double g2 = 2.0 * f * (k1 + 2.0 * k2 * n);
    const double Dp[2][2] = {{sc + g2 * p0 * p0, g2 * p0 * p1}, {g2 * p1 * p0, sc + g2 * p1 * p1}};
    double D[2][3];
    for (int a = 0; a < 2; ++a)
      for (int k = 0; k < 3; ++k) D[a][k] = Dp[a][0] * dpP[0][k] + Dp[a][1] * dpP[1][k];
    const double pp[2] = {p0, p1};
    for (int a = 0; a < 2; ++a) {
      for (int k = 0; k < 3; ++k) {
        J[a][k] = D[a][0] * dR[0][k] + D[a][1] * dR[1][k] + D[a][2] * dR[2][k];
        J[a][3 + k] = D[a][k];
        J[a][9 + k] = D[a][0] * R[0][k] + D[a][1] * R[1][k] + D[a][2] * R[2][k];
      }
      J[a][6] = pp[a] * rad;
      J[a][7] = pp[a] * (f * n);
      J[a][8] = pp[a] * (f * n * n);
    }
  }
}

// Single-call form (standalone residual / Jacobian entry points).
template <bool JAC>
__device__ __forceinline__ void reproject(const double* __restrict__ cam,
                                          const double* __restrict__ X,
                                          const double* __restrict__ q, double r[2],
                                          double J[2][12]) {
  double cr[kCamRec];
  cam_prep(cam, cr);
  reproject_pre<JAC>(cr, X, q, r, J);
}

// The two clamps of BundleAdjustment.py:339-350 (x first, then y on the
// rescaled row), with the chain rule applied to J when JAC.
template <bool JAC>
__device__ __forceinline__ void clamp_rows(double r[2], double J[2][12]) {
#pragma unroll
  for (int comp = 0; comp < 2; ++comp) {
    const double rc = r[comp];
    if (fabs(rc) > kClamp) {
      const double arc = fabs(rc);
      const double half = comp == 0 ? 613.0 : 185.0;
      if constexpr (JAC) {
        const double a = (half * 2.0) / arc;
        double Jc[12];
        for (int k = 0; k < 12; ++k) Jc[k] = J[comp][k];
        for (int row = 0; row < 2; ++row) {
          const double ratio = r[row] / rc;
          for (int k = 0; k < 12; ++k) J[row][k] = a * (J[row][k] - ratio * Jc[k]);
        }
      }
      r[0] = r[0] / arc * half * 2.0;
      r[1] = r[1] / arc * half * 2.0;
    }
  }
}

// Held camera parameters (slam_ba_problem.cam_fixed): bit i of a camera's mask
// word removes column i of the 2 x 9 camera block of its observations, before
// the block enters any product, so the row and column of that parameter in the
// reduced camera system are zero up to the damped diagonal and its step is an
// exact zero.  (After the clamp: its chain rule is per column, 0 stays 0.)
__device__ __forceinline__ void hold_cols(double J[2][12], unsigned fx) {
#pragma unroll
  for (int i = 0; i < 9; ++i)
    if ((fx >> i) & 1u) J[0][i] = J[1][i] = 0.0;
}
// the two-lane form: half H holds camera columns 6 H .. 6 H + 5 (H = 1: 6..8)
template <int H>
__device__ __forceinline__ void hold_cols_half(double Jh[2][6], unsigned fx) {
#pragma unroll
  for (int i = 0; i < (H == 0 ? 6 : 3); ++i)
    if ((fx >> (6 * H + i)) & 1u) Jh[0][i] = Jh[1][i] = 0.0;
}

// The robust loss per observation (slam_ba_problem.loss != 0): robust_weight<NC>
// of robust_loss.hpp, applied after the clamp and hold_cols.

// reproject_pre<true> + clamp_rows<true> split over two lanes by Jacobian
// columns: H = 0 the rotation / translation columns 0..5, H = 1 the f, k1, k2
// and point columns 6..11 (Jh[a][k] = J[a][6 H + k]).  Both halves run the
// forward projection; every value is computed with the same operations in
// the same order as the one-lane form (the clamp's chain rule is per column).
template <int H>
__device__ __forceinline__ void reproject_half(const double* __restrict__ cr,
                                               const double* __restrict__ X,
                                               const double* __restrict__ q, double r[2],
                                               double Jh[2][6]) {
  const double c = cr[0], s = cr[1], omc = cr[2];
  const double v0 = cr[3], v1 = cr[4], v2 = cr[5];
  const double X0 = X[0], X1 = X[1], X2 = X[2];
  const double dot = X0 * v0 + X1 * v1 + X2 * v2;
  const double cx0 = v1 * X2 - v2 * X1;
  const double cx1 = v2 * X0 - v0 * X2;
  const double cx2 = v0 * X1 - v1 * X0;
  const double dk = dot * omc;
  const double RX0 = c * X0 + s * cx0 + dk * v0;
  const double RX1 = c * X1 + s * cx1 + dk * v1;
  const double RX2 = c * X2 + s * cx2 + dk * v2;
  const double P0 = RX0 + cr[26], P1 = RX1 + cr[27], P2 = RX2 + cr[28];
  const double p0 = -P0 / P2, p1 = -P1 / P2;
  const double f = cr[29], k1 = cr[30], k2 = cr[31];
  const double n = p0 * p0 + p1 * p1;
  const double rad = 1.0 + k1 * n + k2 * (n * n);
  const double sc = rad * f;
  r[0] = p0 * sc - q[0];
  r[1] = p1 * sc - q[1];
  const double iz = 1.0 / P2;
  const double dpP[2][3] = {{-iz, 0.0, P0 * iz * iz}, {0.0, -iz, P1 * iz * iz}};
  const double g2 = 2.0 * f * (k1 + 2.0 * k2 * n);
  const double Dp[2][2] = {{sc + g2 * p0 * p0, g2 * p0 * p1}, {g2 * p1 * p0, sc + g2 * p1 * p1}};
  double D[2][3];
  for (int a = 0; a < 2; ++a)
    for (int k = 0; k < 3; ++k) D[a][k] = Dp[a][0] * dpP[0][k] + Dp[a][1] * dpP[1][k];
  if constexpr (H == 0) {
    double dR[3][3];
    if (cr[25] != 0.0) {
      dR[0][0] = 0.0;  dR[0][1] = RX2;  dR[0][2] = -RX1;
      dR[1][0] = -RX2; dR[1][1] = 0.0;  dR[1][2] = RX0;
      dR[2][0] = RX1;  dR[2][1] = -RX0; dR[2][2] = 0.0;
    } else {
      double R[3][3], A[3][3];
      for (int i = 0; i < 9; ++i) {
        R[i / 3][i % 3] = cr[6 + i];
        A[i / 3][i % 3] = cr[15 + i];
      }
      const double Xs[3][3] = {{0.0, -X2, X1}, {X2, 0.0, -X0}, {-X1, X0, 0.0}};
      double B[3][3];
      for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k)
          B[i][k] = Xs[i][0] * A[0][k] + Xs[i][1] * A[1][k] + Xs[i][2] * A[2][k];
      const double inv = cr[24];
      for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k)
          dR[i][k] = (R[i][0] * B[0][k] + R[i][1] * B[1][k] + R[i][2] * B[2][k]) * inv;
    }
    for (int a = 0; a < 2; ++a)
      for (int k = 0; k < 3; ++k) {
        Jh[a][k] = D[a][0] * dR[0][k] + D[a][1] * dR[1][k] + D[a][2] * dR[2][k];
        Jh[a][3 + k] = D[a][k];
      }
  } else {
    double R[3][3];
    for (int i = 0; i < 9; ++i) R[i / 3][i % 3] = cr[6 + i];
    const double pp[2] = {p0, p1};
    for (int a = 0; a < 2; ++a) {
      Jh[a][0] = pp[a] * rad;
      Jh[a][1] = pp[a] * (f * n);
      Jh[a][2] = pp[a] * (f * n * n);
      for (int k = 0; k < 3; ++k) Jh[a][3 + k] = D[a][0] * R[0][k] + D[a][1] * R[1][k] + D[a][2] * R[2][k];
    }
  }
#pragma unroll
  for (int comp = 0; comp < 2; ++comp) {  // clamp_rows<true> on this lane's columns
    const double rc = r[comp];
    if (fabs(rc) > kClamp) {
      const double arc = fabs(rc);
      const double half = comp == 0 ? 613.0 : 185.0;
      const double a = (half * 2.0) / arc;
      double Jc[6];
      for (int k = 0; k < 6; ++k) Jc[k] = Jh[comp][k];
      for (int row = 0; row < 2; ++row) {
        const double ratio = r[row] / rc;
        for (int k = 0; k < 6; ++k) Jh[row][k] = a * (Jh[row][k] - ratio * Jc[k]);
      }
      r[0] = r[0] / arc * half * 2.0;
      r[1] = r[1] / arc * half * 2.0;
    }
  }
}

}  // namespace
