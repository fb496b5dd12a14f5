// The robust loss of one 2-D reprojection residual, shared by bundle adjustment
// (ba_project.hpp) and the pose refinement (pose_refine.hip).
#pragma once

namespace {

// Robust loss per observation (loss != 0, delta = loss_scale):
// with s = |r|^2 of the (clamped) residual and z = s / delta^2, r and the lane's
// NC Jacobian columns (J0, J1: rows 0, 1; 12, a half's 6, or 0 = none) are
// scaled by sqrt(w), w = rho'(z), and delta^2 rho(z) is returned -- the
// observation's term of twice the LM cost, in place of s.  Both lanes of a
// split observation hold the full r, so both form the same w.  After the clamp
// and hold_cols (a held column is 0 and stays 0).  huber with z <= 1 is the
// plain loss exactly: nothing is scaled, s is returned.
template <int NC>
__device__ __forceinline__ double robust_weight(double r[2], double* J0, double* J1, int loss,
                                                double delta) {
  const double s = r[0] * r[0] + r[1] * r[1];
  const double d2 = delta * delta;
  const double z = s / d2;
  double sw, rho;
  if (loss == 1) {         // huber: rho = z | 2 sqrt(z) - 1, w = 1 | 1 / sqrt(z)
    if (z <= 1.0) return s;
    const double q = sqrt(z);
    sw = 1.0 / sqrt(q);
    rho = 2.0 * q - 1.0;
  } else if (loss == 2) {  // soft_l1: rho = 2 (sqrt(1 + z) - 1), w = 1 / sqrt(1 + z)
    const double q = sqrt(1.0 + z);
    sw = 1.0 / sqrt(q);
    rho = 2.0 * z / (q + 1.0);  // = 2 (q - 1) without the cancellation at small z
  } else {                 // cauchy: rho = log(1 + z), w = 1 / (1 + z)
    sw = 1.0 / sqrt(1.0 + z);
    rho = log1p(z);
  }
  r[0] *= sw;
  r[1] *= sw;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    J0[k] *= sw;
    J1[k] *= sw;
  }
  return d2 * rho;
}

}  // namespace
