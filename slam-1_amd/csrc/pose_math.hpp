// Device helpers shared by the pose estimators (geometry.hip: PnP, stereo VO;
// pose_refine.hip): Rodrigues, the reprojection residual with its Gallego-Yezzi
// rotation Jacobian, the general 3x4 projection, the damped 6x6 solve and the
// wave sums of the normal equations.
#pragma once

#include "common.hpp"

namespace {

// cv::Rodrigues (rotation vector -> matrix)
__device__ inline void rodrigues(const double r[3], double R[9]) {
  const double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  if (th < 2.220446049250313e-16) {
    R[0] = 1; R[1] = 0; R[2] = 0; R[3] = 0; R[4] = 1; R[5] = 0; R[6] = 0; R[7] = 0; R[8] = 1;
    return;
  }
  const double c = cos(th), s = sin(th), c1 = 1.0 - c, it = 1.0 / th;
  const double x = r[0] * it, y = r[1] * it, z = r[2] * it;
  R[0] = c + c1 * x * x; R[1] = c1 * x * y - s * z; R[2] = c1 * x * z + s * y;
  R[3] = c1 * x * y + s * z; R[4] = c + c1 * y * y; R[5] = c1 * y * z - s * x;
  R[6] = c1 * x * z - s * y; R[7] = c1 * y * z + s * x; R[8] = c + c1 * z * z;
}

struct Cam {
  double fx, fy, cx, cy;
};

// D = d(R(w) X)/dw with R = R(w) and RX = R X given: Gallego & Yezzi,
// -R [X]x (w w^T + (R^T - I)[w]x) / |w|^2, and -[RX]x at w = 0.
__device__ inline void drot_left(const double w[3], const double R[9], double X0, double X1,
                                 double X2, double RX0, double RX1, double RX2, double D[3][3]) {
  const double w0 = w[0], w1 = w[1], w2 = w[2];
  const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
  if (th2 < 1e-24) {
    D[0][0] = 0; D[0][1] = RX2; D[0][2] = -RX1;
    D[1][0] = -RX2; D[1][1] = 0; D[1][2] = RX0;
    D[2][0] = RX1; D[2][1] = -RX0; D[2][2] = 0;
  } else {
    const double W[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
    const double wv[3] = {w0, w1, w2};
    double Am[3][3];
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) {
        double acc = wv[i] * wv[k];
        for (int j = 0; j < 3; ++j) acc += R[3 * j + i] * W[j][k];
        Am[i][k] = acc - W[i][k];
      }
    const double Xs[3][3] = {{0.0, -X2, X1}, {X2, 0.0, -X0}, {-X1, X0, 0.0}};
    double B[3][3];
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k)
        B[i][k] = Xs[i][0] * Am[0][k] + Xs[i][1] * Am[1][k] + Xs[i][2] * Am[2][k];
    const double inv = -1.0 / th2;
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k)
        D[i][k] = (R[3 * i] * B[0][k] + R[3 * i + 1] * B[1][k] + R[3 * i + 2] * B[2][k]) * inv;
  }
}

// reprojection residual of one point and (optionally) its 2x6 Jacobian wrt (r, t)
template <bool JAC>
__device__ inline void pnp_residual(const double p[6], const double R[9], const double* Q,
                                    const double* q, const Cam& K, double r[2], double J[2][6]) {
  const double X0 = Q[0], X1 = Q[1], X2 = Q[2];
  const double RX0 = R[0] * X0 + R[1] * X1 + R[2] * X2;
  const double RX1 = R[3] * X0 + R[4] * X1 + R[5] * X2;
  const double RX2 = R[6] * X0 + R[7] * X1 + R[8] * X2;
  const double Xc = RX0 + p[3], Yc = RX1 + p[4], Zc = RX2 + p[5];
  const double iz = 1.0 / Zc;
  r[0] = K.fx * (Xc * iz) + K.cx - q[0];
  r[1] = K.fy * (Yc * iz) + K.cy - q[1];
  if constexpr (JAC) {
    const double du[3] = {K.fx * iz, 0.0, -K.fx * Xc * iz * iz};
    const double dv[3] = {0.0, K.fy * iz, -K.fy * Yc * iz * iz};
    double D[3][3];
    drot_left(p, R, X0, X1, X2, RX0, RX1, RX2, D);
    for (int k = 0; k < 3; ++k) {
      J[0][k] = du[0] * D[0][k] + du[1] * D[1][k] + du[2] * D[2][k];
      J[1][k] = dv[0] * D[0][k] + dv[1] * D[1][k] + dv[2] * D[2][k];
      J[0][3 + k] = du[k];
      J[1][3 + k] = dv[k];
    }
  }
}

// X -> (u, v) with P (3x4 row-major); a0/a1: d(u, v)/dX when JAC
template <bool JAC>
__device__ inline void vo_project(const double* P, const double X[3], double uv[2], double a[2][3]) {
  const double x0 = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
  const double x1 = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
  const double x2 = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
  const double iz = 1.0 / x2;
  uv[0] = x0 * iz;
  uv[1] = x1 * iz;
  if constexpr (JAC) {
    for (int k = 0; k < 3; ++k) {
      a[0][k] = (P[k] - uv[0] * P[8 + k]) * iz;
      a[1][k] = (P[4 + k] - uv[1] * P[8 + k]) * iz;
    }
  }
}

// Solve (H + lam diag(H)) d = -g for the 6x6 SPD system (Cholesky); false on failure.
__device__ inline bool solve6(const double H[21], const double g[6], double lam, double d[6]) {
  double A[6][6];
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j) {
      A[i][j] = H[k];
      A[j][i] = H[k];
      ++k;
    }
  for (int i = 0; i < 6; ++i) A[i][i] += lam * fmax(A[i][i], 1e-12);
  for (int j = 0; j < 6; ++j) {
    double s = A[j][j];
    for (int p = 0; p < j; ++p) s -= A[j][p] * A[j][p];
    if (!(s > 0.0)) return false;
    A[j][j] = sqrt(s);
    for (int i = j + 1; i < 6; ++i) {
      double t = A[i][j];
      for (int p = 0; p < j; ++p) t -= A[i][p] * A[j][p];
      A[i][j] = t / A[j][j];
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double t = -g[i];
    for (int p = 0; p < i; ++p) t -= A[i][p] * y[p];
    y[i] = t / A[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double t = y[i];
    for (int p = i + 1; p < 6; ++p) t -= A[p][i] * d[p];
    d[i] = t / A[i][i];
  }
  return true;
}

// Sum over the 64 lanes of a wave, every lane ends with the total (xor butterfly).
__device__ __forceinline__ double wave_allsum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Sums of 32 values over the 64 lanes of a wave, every lane ends with all 32
// totals (v[k] = total k).  Reduce-scatter by halving: at offset 32, 16, .., 2
// a lane keeps the half of its values its partner does not (one shuffle per
// kept value: 16 + 8 + 4 + 2 + 1, then one at offset 1), so total j ends on
// lanes 2j and 2j+1 and is broadcast by v_readlane -- 32 double shuffles
// instead of 6 per value of the xor butterfly.
__device__ __forceinline__ double readlane_d(double x, int l) {
  const unsigned long long u = __double_as_longlong(x);
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)u, l);
  const unsigned hi = __builtin_amdgcn_readlane((unsigned)(u >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
template <int OFF>
__device__ __forceinline__ void allsum_halve(double (&v)[32], int lane) {
  constexpr int half = OFF / 2;
  const bool hi = (lane & OFF) != 0;
#pragma unroll
  for (int k = 0; k < half; ++k) {
    const double send = hi ? v[k] : v[k + half];
    const double keep = hi ? v[k + half] : v[k];
    v[k] = keep + __shfl_xor(send, OFF, 64);
  }
}
__device__ __forceinline__ void wave_allsum32(double (&v)[32]) {
  const int lane = threadIdx.x & 63;
  allsum_halve<32>(v, lane);
  allsum_halve<16>(v, lane);
  allsum_halve<8>(v, lane);
  allsum_halve<4>(v, lane);
  allsum_halve<2>(v, lane);
  const double tot = v[0] + __shfl_xor(v[0], 1, 64);
#pragma unroll
  for (int j = 0; j < 32; ++j) v[j] = readlane_d(tot, 2 * j);
}

}  // namespace
