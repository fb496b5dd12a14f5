// The per-camera half of the BAL projection: shared by ba.hip (k_reset, the
// linearisers and the back substitution read its records) and by the solve
// epilogue, which prepares the trial cameras.
#pragma once

#include "ba_layout.hpp"

namespace {

// Residual (proj - q) of BundleAdjustment.py:317-337 with the operation order
// of the numpy code, and optionally its analytic 2x12 Jacobian.
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

}  // namespace
