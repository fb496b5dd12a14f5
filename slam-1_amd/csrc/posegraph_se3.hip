// SE(3) pose graph (include/slam355.h "SE(3) pose graph"):
// weighted relative-pose edges between arbitrary keyframes, Levenberg-Marquardt
// on the device with the BA's rules and state slots.  Per iteration:
//   k_pg_lin       one lane per edge: e, J_i, J_j, A_k, held columns, robust
//                  weight -> edge record (r~, J~_i, J~_j)
//   k_pg_zero      the stored tiles of the row profile <- 0 (unit diagonal on
//                  padding rows), b, g, D <- 0, the failure flag cleared
//   k_pg_assemble  one workgroup per pose (H_ii, g_i, D_i) and per unique pose
//                  pair (H_hi,lo): fixed-order sums over the host's lists, no
//                  floating-point atomics; written damped into 64x64 lower tiles
//                  of 10 poses each
//   k_pg_panel / k_pg_update   per tile column k of the row profile ("skyline"):
//                  factor + inverse of the diagonal tile (tile_chol_inv_blk),
//                  y_k = L_kk^-1 b_k, L_Ik = A_Ik L_kk^-T over the column's
//                  panel rows; then A_IJ -= L_Ik L_Jk^T over its update pairs
//                  (b_I -= L_Ik y_k on the diagonal ones)
//   k_pg_back      x_k = L_kk^-T (y_k - sum_I L_Ik^T x_I), columns in reverse
//   k_pg_trial     x_trial = x + delta into the other buffer, the terms of
//                  pred, and every edge's cost at the trial point
//   k_pg_decide    fixed-tree sums of both, then the BA's accept / lambda rules
// Ordering comes from the stream alone: no kernel waits on another workgroup.
// The covariance of the poses and the gate of candidate edges
// reuse the factor at lambda = 0: "covariance" below.
#include "tile_f64.hpp"

#include <algorithm>
#include <vector>

namespace {

constexpr int kPgMagic = 0x50473031;
constexpr int kPgHdr = 16;    // ints of the schedule's header
constexpr int kPgTP = 10;     // poses per tile (60 of 64 rows)
constexpr int kPgRec = 80;    // doubles per edge record: r~ 6, J~_i 36, J~_j 36, 2 of padding
constexpr int kPgWG = 64;     // k_pg_lin / k_pg_assemble / k_pg_trial workgroup
constexpr int kPgSumWG = 1024;
constexpr double kPgSmall = 0.05;  // below: the series of the SO(3) coefficients
constexpr double kPgLamMin = 1e-16, kPgLamMax = 1e32;

struct PgSched {  // offsets (ints) inside the schedule, from the sizes alone
  long long first, rowoff, pose_ptr, pose_ent, pair_ptr, pair_ij, pair_ent, col_ptr, upd_ptr, lists;
  __host__ __device__ PgSched(int N, int E, int T, int P) {
    first = kPgHdr;
    rowoff = first + T;
    pose_ptr = rowoff + T + 1;
    pose_ent = pose_ptr + N + 1;
    pair_ptr = pose_ent + 2ll * E;
    pair_ij = pair_ptr + P + 1;
    pair_ent = pair_ij + 2ll * P;
    col_ptr = pair_ent + E;
    upd_ptr = col_ptr + T + 1;
    lists = upd_ptr + T + 1;  // panel rows of every column, then the update pairs
  }
};

struct PgLayout {  // doubles inside ws
  long long rec, tiles, dinv, b, y, x, g, d, cterm, pterm, flag, total;
  __host__ __device__ PgLayout(int N, int E, int T, long long n_tiles) {
    rec = 0;
    tiles = rec + (long long)kPgRec * E;       // stored tiles, row-major 64x64 each
    dinv = tiles + n_tiles * kTB * kTB;        // L_kk^-1 per tile column
    b = dinv + (long long)T * kTB * kTB;
    y = b + (long long)T * kTB;
    x = y + (long long)T * kTB;
    g = x + (long long)T * kTB;                // g and D = clip(diag H) in tile rows
    d = g + (long long)T * kTB;
    cterm = d + (long long)T * kTB;            // [E] cost terms at the trial point
    pterm = cterm + E;                         // [6 N] terms of pred
    flag = pterm + 6ll * N;                    // (int) the factor failed
    total = flag + 8;
  }
};

// what the kernels need of the problem, resolved on the host
struct PgArgs {
  slam_pg_problem p;
  int T, P;
  long long n_tiles;
};

__device__ __forceinline__ int pg_cur(const slam_pg_problem& p) {
  return p.state != nullptr && p.state[SLAM_BA_ST_CUR] != 0.0 ? 1 : 0;
}
__device__ __forceinline__ int pg_row(int pose) { return (pose / kPgTP) * kTB + (pose % kPgTP) * 6; }
__device__ __forceinline__ bool pg_failed(const double* ws, const PgLayout& L) {
  return *reinterpret_cast<const volatile int*>(ws + L.flag) != 0;
}

// The stored tiles of the row profile as the tile steps of tile_f64.hpp address
// them: row I keeps its tiles first[I] .. I packed from tile index rowoff[I].
// ld is an int on purpose (the steps take a row offset's type from it): with
// 64-bit row offsets k_pg_back waits after every load of its row loop and a
// full-profile iteration takes 5.6 ms instead of 3.5 (profiles/tile_steps/).
struct SkylineTiles {
  double* tiles;
  const int32_t *first, *rowoff;
  static constexpr int ld = kTB;
  __device__ __forceinline__ SkylineTiles(const slam_pg_problem& p, const PgSched& S, const PgLayout& L)
      : tiles(p.ws + L.tiles), first(p.sched + S.first), rowoff(p.sched + S.rowoff) {}
  __device__ __forceinline__ double* at(int I, int J) const {
    return tiles + (long long)(rowoff[I] + J - first[I]) * kTB * kTB;
  }
};

// ---------------------------------------------------------------- SO(3)
// a = sin(th)/th, b = (1 - cos th)/th^2, c = (th - sin th)/th^3 from th^2
__device__ __forceinline__ void so3_abc(double t2, double& a, double& b, double& c) {
  if (t2 < kPgSmall * kPgSmall) {
    a = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0));
    b = 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0 * (1.0 - t2 / 56.0));
    c = 1.0 / 6.0 - t2 / 120.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0));
  } else {
    const double th = sqrt(t2), s = sin(th), h = sin(0.5 * th);
    a = s / th;
    b = 2.0 * h * h / t2;
    c = (th - s) / (t2 * th);
  }
}
// k of J_r^-1 = I + [phi]x / 2 + k [phi]x^2: (1 - (th/2) cot(th/2)) / th^2
__device__ __forceinline__ double so3_k(double t2) {
  if (t2 < kPgSmall * kPgSmall) return 1.0 / 12.0 + t2 / 720.0 * (1.0 + t2 / 42.0 * (1.0 + t2 / 40.0));
  const double th = sqrt(t2), hs = sin(0.5 * th), hc = cos(0.5 * th);
  return (1.0 - 0.5 * th * hc / hs) / t2;
}
// M = I + p [r]x + q [r]x^2  ([r]x^2 = r r^T - |r|^2 I), row-major
__device__ __forceinline__ void so3_poly(const double r[3], double t2, double p, double q, double M[9]) {
  M[0] = 1.0 + q * (r[0] * r[0] - t2);
  M[4] = 1.0 + q * (r[1] * r[1] - t2);
  M[8] = 1.0 + q * (r[2] * r[2] - t2);
  const double q01 = q * (r[0] * r[1]), q02 = q * (r[0] * r[2]), q12 = q * (r[1] * r[2]);
  M[1] = q01 - p * r[2];
  M[3] = q01 + p * r[2];
  M[2] = q02 + p * r[1];
  M[6] = q02 - p * r[1];
  M[5] = q12 - p * r[0];
  M[7] = q12 + p * r[0];
}
__device__ __forceinline__ double dot3(const double a[3]) { return a[0] * a[0] + a[1] * a[1] + a[2] * a[2]; }
__device__ __forceinline__ void so3_exp(const double r[3], double R[9]) {
  const double t2 = dot3(r);
  double a, b, c;
  so3_abc(t2, a, b, c);
  so3_poly(r, t2, a, b, R);
}
__device__ __forceinline__ void so3_jr(const double r[3], double J[9]) {  // right Jacobian
  const double t2 = dot3(r);
  double a, b, c;
  so3_abc(t2, a, b, c);
  so3_poly(r, t2, -b, c, J);
}
__device__ __forceinline__ void so3_jr_inv(const double r[3], double J[9]) {
  const double t2 = dot3(r);
  so3_poly(r, t2, 0.5, so3_k(t2), J);
}
// rotation vector of R, angle in [0, pi]
__device__ __forceinline__ void so3_log(const double R[9], double phi[3]) {
  const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};  // sin(th) axis
  const double s2 = dot3(v), s = sqrt(s2);
  const double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
  const double th = atan2(s, c);
  if (c < 0.0 && s < 1e-3) {
    // within 1e-3 of pi: the axis from the symmetric part, R + R^T = 2 c I + 2 (1 - c) n n^T
    // (the largest component positive, the others signed by its row; then towards v)
    const double den = 1.0 - c;
    double n0 = sqrt(fmax((R[0] - c) / den, 0.0)), n1 = sqrt(fmax((R[4] - c) / den, 0.0)),
           n2 = sqrt(fmax((R[8] - c) / den, 0.0));
    const double s01 = R[1] + R[3], s02 = R[2] + R[6], s12 = R[5] + R[7];
    if (n0 >= n1 && n0 >= n2) {
      if (s01 < 0.0) n1 = -n1;
      if (s02 < 0.0) n2 = -n2;
    } else if (n1 >= n2) {
      if (s01 < 0.0) n0 = -n0;
      if (s12 < 0.0) n2 = -n2;
    } else {
      if (s02 < 0.0) n0 = -n0;
      if (s12 < 0.0) n1 = -n1;
    }
    const double sg = (v[0] * n0 + v[1] * n1) + v[2] * n2 < 0.0 ? -th : th;
    phi[0] = sg * n0;
    phi[1] = sg * n1;
    phi[2] = sg * n2;
    return;
  }
  double f;  // th / sin(th)
  if (c > 0.0 && s < kPgSmall) f = 1.0 + s2 / 6.0 * (1.0 + s2 * 9.0 / 20.0 * (1.0 + s2 * 25.0 / 42.0));
  else f = th / s;
  for (int q = 0; q < 3; ++q) phi[q] = f * v[q];
}
// C = A B, C = A^T B (3x3 row-major)
__device__ __forceinline__ void mm3(const double A[9], const double B[9], double C[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ void mtm3(const double A[9], const double B[9], double C[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[i] * B[j] + A[3 + i] * B[3 + j]) + A[6 + i] * B[6 + j];
}
__device__ __forceinline__ void mtv3(const double A[9], const double v[3], double o[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = (A[i] * v[0] + A[3 + i] * v[1]) + A[6 + i] * v[2];
}

// ---------------------------------------------------------------- one edge
// e = [Log(R_z^T R_i^T R_j); R_z^T (R_i^T (t_j - t_i) - t_z)], r = A e; JAC: the
// raw 6x6 Jacobians d e / d x_i, d e / d x_j (row-major) with the held columns zero
template <bool JAC>
__device__ __forceinline__ void pg_edge_raw(const double xi[6], const double xj[6], const double z[6],
                                            unsigned fi, unsigned fj, double e[6], double Ji[36],
                                            double Jj[36]) {
  double Ri[9], Rj[9], Rz[9], Rij[9], RE[9];
  so3_exp(xi, Ri);
  so3_exp(xj, Rj);
  so3_exp(z, Rz);
  const double dt[3] = {xj[3] - xi[3], xj[4] - xi[4], xj[5] - xi[5]};
  double u[3];
  mtv3(Ri, dt, u);
  mtm3(Ri, Rj, Rij);
  mtm3(Rz, Rij, RE);
  so3_log(RE, e);
  const double uz[3] = {u[0] - z[3], u[1] - z[4], u[2] - z[5]};
  mtv3(Rz, uz, e + 3);
  if constexpr (JAC) {
    double Jri[9], Jrj[9], Jinv[9], M[9], dRi[9], dRj[9], W[9], dTr[9], RzRiT[9];
    so3_jr(xi, Jri);
    so3_jr(xj, Jrj);
    so3_jr_inv(e, Jinv);
    mm3(Jinv, Jrj, dRj);          // d e_rot / d r_j
    mtm3(Rij, Jri, M);            // R_j^T R_i J_r(r_i)
    mm3(Jinv, M, dRi);            // -(d e_rot / d r_i)
    const double ux[9] = {0.0, -u[2], u[1], u[2], 0.0, -u[0], -u[1], u[0], 0.0};
    mm3(ux, Jri, W);
    mtm3(Rz, W, dTr);             // d t_E / d r_i
    // R_z^T R_i^T = (R_i R_z)^T
    double RiRz[9];
    mm3(Ri, Rz, RiRz);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) RzRiT[3 * a + b] = RiRz[3 * b + a];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        Ji[6 * a + b] = -dRi[3 * a + b];
        Ji[6 * a + 3 + b] = 0.0;
        Ji[6 * (a + 3) + b] = dTr[3 * a + b];
        Ji[6 * (a + 3) + 3 + b] = -RzRiT[3 * a + b];
        Jj[6 * a + b] = dRj[3 * a + b];
        Jj[6 * a + 3 + b] = 0.0;
        Jj[6 * (a + 3) + b] = 0.0;
        Jj[6 * (a + 3) + 3 + b] = RzRiT[3 * a + b];
      }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      if ((fi >> c) & 1u)
#pragma unroll
        for (int n = 0; n < 6; ++n) Ji[6 * n + c] = 0.0;
      if ((fj >> c) & 1u)
#pragma unroll
        for (int n = 0; n < 6; ++n) Jj[6 * n + c] = 0.0;
    }
  }
}

// sqrt(w) and the cost term delta^2 rho(z) of s = |r|^2 (the BA's robust_weight:
// huber with z <= 1 and the linear loss scale nothing and return s)
__device__ __forceinline__ double pg_robust(double s, int loss, double delta, double& sw) {
  sw = 1.0;
  if (loss == 0) return s;
  const double d2 = delta * delta;
  const double z = s / d2;
  double rho;
  if (loss == 1) {
    if (z <= 1.0) return s;
    const double q = sqrt(z);
    sw = 1.0 / sqrt(q);
    rho = 2.0 * q - 1.0;
  } else if (loss == 2) {
    const double q = sqrt(1.0 + z);
    sw = 1.0 / sqrt(q);
    rho = 2.0 * z / (q + 1.0);
  } else {
    sw = 1.0 / sqrt(1.0 + z);
    rho = log1p(z);
  }
  return d2 * rho;
}

// o = A v (6x6 row-major A in memory), sums in index order
__device__ __forceinline__ void pg_av(const double* __restrict__ A, const double v[6], double o[6]) {
#pragma unroll
  for (int m = 0; m < 6; ++m) {
    double s = A[6 * m] * v[0];
#pragma unroll
    for (int n = 1; n < 6; ++n) s += A[6 * m + n] * v[n];
    o[m] = s;
  }
}

// The lineariser: one lane per edge.  Outputs (any may be null): raw e, r~,
// J~_i, J~_j (strides in doubles).  (The cost is summed by k_pg_trial's terms.)
template <bool JAC>
__global__ __launch_bounds__(kPgWG) void k_pg_lin(slam_pg_problem p, double* __restrict__ oe, int se,
                                                  double* __restrict__ orr, int sr,
                                                  double* __restrict__ oji, double* __restrict__ ojj,
                                                  int sj) {
  const int k = blockIdx.x * kPgWG + threadIdx.x;
  if (k >= p.n_edges) return;
  const double* x = p.poses[pg_cur(p)];
  const int i = p.edge_ij[2 * k], j = p.edge_ij[2 * k + 1];
  double xi[6], xj[6], z[6], e[6], r[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    xi[q] = x[6 * i + q];
    xj[q] = x[6 * j + q];
    z[q] = p.meas[6ll * k + q];
  }
  const unsigned fi = p.pose_fixed ? p.pose_fixed[i] : 0u, fj = p.pose_fixed ? p.pose_fixed[j] : 0u;
  double Ji[JAC ? 36 : 1], Jj[JAC ? 36 : 1];
  pg_edge_raw<JAC>(xi, xj, z, fi, fj, e, Ji, Jj);
  const double* A = p.sqrt_info + 36ll * k;
  pg_av(A, e, r);
  double s = r[0] * r[0];
#pragma unroll
  for (int q = 1; q < 6; ++q) s += r[q] * r[q];
  double sw;
  pg_robust(s, p.loss, p.loss_scale, sw);
  const bool scale = sw != 1.0;
  if (oe != nullptr)
#pragma unroll
    for (int q = 0; q < 6; ++q) oe[(long long)se * k + q] = e[q];
  if (orr != nullptr)
#pragma unroll
    for (int q = 0; q < 6; ++q) orr[(long long)sr * k + q] = scale ? r[q] * sw : r[q];
  if constexpr (JAC) {
    // J~ = sqrt(w) A J, one output column at a time
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const double* J = side ? Jj : Ji;
      double* o = (side ? ojj : oji) + (long long)sj * k;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const double col[6] = {J[c], J[6 + c], J[12 + c], J[18 + c], J[24 + c], J[30 + c]};
        double ac[6];
        pg_av(A, col, ac);
#pragma unroll
        for (int m = 0; m < 6; ++m) o[6 * m + c] = scale ? ac[m] * sw : ac[m];
      }
    }
  }
}

// ---------------------------------------------------------------- assembly
// stored tile index -> (I, J): rowoff is ascending
__device__ __forceinline__ void pg_tile_of(const int32_t* first, const int32_t* rowoff, int T, int idx,
                                           int& I, int& J) {
  int lo = 0, hi = T - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rowoff[mid] <= idx) lo = mid;
    else hi = mid - 1;
  }
  I = lo;
  J = first[I] + idx - rowoff[I];
}

__global__ __launch_bounds__(kTlWG) void k_pg_zero(PgArgs a) {
  const slam_pg_problem& p = a.p;
  const PgSched S(p.n_poses, p.n_edges, a.T, a.P);
  const PgLayout L(p.n_poses, p.n_edges, a.T, a.n_tiles);
  int I, J;
  pg_tile_of(p.sched + S.first, p.sched + S.rowoff, a.T, blockIdx.x, I, J);
  double* tile = p.ws + L.tiles + (long long)blockIdx.x * kTB * kTB;
  const int t = threadIdx.x;
  const int rows = 6 * min(kPgTP, p.n_poses - kPgTP * I);  // rows of H in tile row I; the rest is padding
  for (int e = t; e < kTB * kTB; e += kTlWG) {
    const int r = e >> 6, c = e & 63;
    tile[e] = (I == J && r == c && r >= rows) ? 1.0 : 0.0;
  }
  if (I == J && t < kTB) {
    p.ws[L.b + I * kTB + t] = 0.0;
    p.ws[L.g + I * kTB + t] = 0.0;
    p.ws[L.d + I * kTB + t] = 0.0;
  }
  if (blockIdx.x == 0 && t == 0) *reinterpret_cast<int*>(p.ws + L.flag) = 0;
}

// blockIdx.x < N: pose i -> H_ii + lambda D_i, g_i, D_i; else pair q -> H_hi,lo.
// Thread (a, b) of 36 sums its entry over the list in list order, rows m in order.
// COV (the covariance's factor at lambda = 0): no damping, D <- diag H itself, and
// an exact 1.0 (in both) on the diagonal of a held parameter, whose row and
// column are exact zeros.
template <bool COV>
__global__ __launch_bounds__(kPgWG) void k_pg_assemble(PgArgs a) {
  const slam_pg_problem& p = a.p;
  const PgSched S(p.n_poses, p.n_edges, a.T, a.P);
  const PgLayout L(p.n_poses, p.n_edges, a.T, a.n_tiles);
  const int32_t* first = p.sched + S.first;
  const int32_t* rowoff = p.sched + S.rowoff;
  const double* rec = p.ws + L.rec;
  const int t = threadIdx.x;
  const int ea = t / 6, eb = t % 6;
  if ((int)blockIdx.x < p.n_poses) {
    const int i = blockIdx.x;
    const int32_t* ent = p.sched + S.pose_ent;
    const int e0 = p.sched[S.pose_ptr + i], e1 = p.sched[S.pose_ptr + i + 1];
    const int I = i / kPgTP, row = pg_row(i);
    if (t < 36) {
      double h = 0.0;
      for (int q = e0; q < e1; ++q) {
        const double* Jt = rec + (long long)kPgRec * (ent[q] >> 1) + 6 + 36 * (ent[q] & 1);
#pragma unroll
        for (int m = 0; m < 6; ++m) h += Jt[6 * m + ea] * Jt[6 * m + eb];
      }
      double* tile = p.ws + L.tiles + (long long)(rowoff[I] + I - first[I]) * kTB * kTB;
      const int lr = row - I * kTB;
      if (ea == eb) {
        if constexpr (COV) {
          if (p.pose_fixed != nullptr && ((p.pose_fixed[i] >> ea) & 1u)) h = 1.0;
          p.ws[L.d + row + ea] = h;
        } else {
          const double d = clampd(h);
          p.ws[L.d + row + ea] = d;
          h += p.state[SLAM_BA_ST_LAMBDA] * d;
        }
      }
      tile[(lr + ea) * kTB + lr + eb] = h;
    } else if (t < 42) {
      const int c = t - 36;
      double g = 0.0;
      for (int q = e0; q < e1; ++q) {
        const double* R = rec + (long long)kPgRec * (ent[q] >> 1);
        const double* Jt = R + 6 + 36 * (ent[q] & 1);
#pragma unroll
        for (int m = 0; m < 6; ++m) g += Jt[6 * m + c] * R[m];
      }
      p.ws[L.g + row + c] = -g;
      p.ws[L.b + row + c] = -g;
    }
    return;
  }
  const int q = blockIdx.x - p.n_poses;
  if (t >= 36) return;
  const int lo = p.sched[S.pair_ij + 2 * q], hi = p.sched[S.pair_ij + 2 * q + 1];
  const int32_t* ent = p.sched + S.pair_ent;
  const int e0 = p.sched[S.pair_ptr + q], e1 = p.sched[S.pair_ptr + q + 1];
  double h = 0.0;
  for (int u = e0; u < e1; ++u) {
    const int flip = ent[u] & 1;  // the edge's i is the pair's hi
    const double* R = rec + (long long)kPgRec * (ent[u] >> 1) + 6;
    const double* Jhi = R + (flip ? 0 : 36);
    const double* Jlo = R + (flip ? 36 : 0);
#pragma unroll
    for (int m = 0; m < 6; ++m) h += Jhi[6 * m + ea] * Jlo[6 * m + eb];
  }
  const int I = hi / kPgTP, J = lo / kPgTP;
  double* tile = p.ws + L.tiles + (long long)(rowoff[I] + J - first[I]) * kTB * kTB;
  tile[(pg_row(hi) - I * kTB + ea) * kTB + pg_row(lo) - J * kTB + eb] = h;
}

// ---------------------------------------------------------------- skyline factor
// Column k: workgroup 0 factors the diagonal tile (L_kk^-1 -> dinv, y_k =
// L_kk^-1 b_k); workgroup 1 + u forms L_Ik = A_Ik L_kk^-T for the u-th panel
// row I (each factors the diagonal tile itself, as k_cov_panel does).
__global__ __launch_bounds__(kTlWG) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_pg_panel(PgArgs a, int k) {
  const slam_pg_problem& p = a.p;
  const PgSched S(p.n_poses, p.n_edges, a.T, a.P);
  const PgLayout L(p.n_poses, p.n_edges, a.T, a.n_tiles);
  const int I = blockIdx.x == 0 ? k : p.sched[S.lists + p.sched[S.col_ptr + k] + blockIdx.x - 1];
  const int rows = 6 * min(kPgTP, p.n_poses - kPgTP * k);
  int* fail = reinterpret_cast<int*>(p.ws + L.flag);
  tile_panel(SkylineTiles(p, S, L), k, I, (rows + 15) >> 4, fail,
             PanelSolveDiag{p.ws + L.dinv + (long long)k * kTB * kTB, p.ws + L.b + k * kTB, p.ws + L.y + k * kTB,
                            fail});
}

// Column k's update pair u = (I, J), I >= J > k: A_IJ -= L_Ik L_Jk^T, and on a
// diagonal pair b_I -= L_Ik y_k.
__global__ __launch_bounds__(kTlWG) void k_pg_update(PgArgs a, int k) {
  const slam_pg_problem& p = a.p;
  const PgSched S(p.n_poses, p.n_edges, a.T, a.P);
  const PgLayout L(p.n_poses, p.n_edges, a.T, a.n_tiles);
  if (pg_failed(p.ws, L)) return;
  // (the pairs follow the panel rows of all columns: header word 6 of them)
  const int32_t* up = p.sched + S.lists + p.sched[6] + 2ll * (p.sched[S.upd_ptr + k] + blockIdx.x);
  tile_update<true>(SkylineTiles(p, S, L), up[0], up[1], k, p.ws + L.y, p.ws + L.b);
}

// x_k = L_kk^-T (y_k - sum_I L_Ik^T x_I), I over column k's panel rows
__global__ __launch_bounds__(kTlWG) void k_pg_back(PgArgs a, int k) {
  const slam_pg_problem& p = a.p;
  const PgSched S(p.n_poses, p.n_edges, a.T, a.P);
  const PgLayout L(p.n_poses, p.n_edges, a.T, a.n_tiles);
  if (pg_failed(p.ws, L)) return;
  const int r0 = p.sched[S.col_ptr + k], r1 = p.sched[S.col_ptr + k + 1];
  tile_back(SkylineTiles(p, S, L), k, r1 - r0, [&](int u) { return p.sched[S.lists + r0 + u]; },
            p.ws + L.dinv + (long long)k * kTB * kTB, p.ws + L.y, p.ws + L.x);
}

// ---------------------------------------------------------------- trial and decide
// parameter q of pose i at the trial point: a held one is copied, the others
// take the step (a failed factor: the zero step)
__device__ __forceinline__ double pg_trial_param(const slam_pg_problem& p, const double* x, const double* dx,
                                                 bool step, int i, int q) {
  const double v = x[6 * i + q];
  if (!step || (p.pose_fixed != nullptr && ((p.pose_fixed[i] >> q) & 1u))) return v;
  return v + dx[pg_row(i) + q];
}

// step != 0: lanes < 6 N write x_trial and their term of 2 pred; lanes < E the
// cost term of their edge at the trial point.  step == 0 (reset): the cost
// terms at the live point only.
__global__ __launch_bounds__(kPgWG) void k_pg_trial(PgArgs a, int step) {
  const slam_pg_problem& p = a.p;
  const PgLayout L(p.n_poses, p.n_edges, a.T, a.n_tiles);
  const int cur = pg_cur(p);
  const double* x = p.poses[cur];
  const double* dx = p.ws + L.x;
  const bool mv = step != 0 && !pg_failed(p.ws, L);
  const int t = blockIdx.x * kPgWG + threadIdx.x;
  if (step != 0 && t < 6 * p.n_poses) {
    const int i = t / 6, q = t % 6;
    const double v = pg_trial_param(p, x, dx, mv, i, q);
    p.poses[cur ^ 1][t] = v;
    const double d = mv ? dx[pg_row(i) + q] : 0.0;
    p.ws[L.pterm + t] = d * (p.state[SLAM_BA_ST_LAMBDA] * p.ws[L.d + pg_row(i) + q] * d + p.ws[L.g + pg_row(i) + q]);
  }
  if (t < p.n_edges) {
    const int i = p.edge_ij[2 * t], j = p.edge_ij[2 * t + 1];
    double xi[6], xj[6], z[6], e[6], r[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      xi[q] = pg_trial_param(p, x, dx, mv, i, q);
      xj[q] = pg_trial_param(p, x, dx, mv, j, q);
      z[q] = p.meas[6ll * t + q];
    }
    pg_edge_raw<false>(xi, xj, z, 0u, 0u, e, nullptr, nullptr);
    pg_av(p.sqrt_info + 36ll * t, e, r);
    double s = r[0] * r[0];
#pragma unroll
    for (int q = 1; q < 6; ++q) s += r[q] * r[q];
    double sw;
    p.ws[L.cterm + t] = pg_robust(s, p.loss, p.loss_scale, sw);
  }
}

// strided partial sums in index order, then block_sum's fixed tree
__device__ __forceinline__ double pg_sum(const double* v, long long n, double* lds) {
  double s = 0.0;
  for (long long q = threadIdx.x; q < n; q += kPgSumWG) s += v[q];
  return block_sum(s, lds);
}

// decide == 0 (reset): COST <- the summed cost terms.  Else the BA's lm_decide.
__global__ __launch_bounds__(kPgSumWG) void k_pg_decide(PgArgs a, int decide) {
  const slam_pg_problem& p = a.p;
  const PgLayout L(p.n_poses, p.n_edges, a.T, a.n_tiles);
  __shared__ double lds[kPgSumWG / 64];
  const double c2 = pg_sum(p.ws + L.cterm, p.n_edges, lds);
  const double p2 = decide ? pg_sum(p.ws + L.pterm, 6ll * p.n_poses, lds) : 0.0;
  if (threadIdx.x != 0) return;
  double* state = p.state;
  if (!decide) {
    state[SLAM_BA_ST_COST] = 0.5 * c2;
    return;
  }
  const bool fail = pg_failed(p.ws, L);
  const double cost = state[SLAM_BA_ST_COST];
  const double cost_new = 0.5 * c2;
  const double pred = 0.5 * p2;
  const double rho = (!fail && pred > 0.0) ? (cost - cost_new) / pred : -1.0;
  double lam = state[SLAM_BA_ST_LAMBDA], nu = state[SLAM_BA_ST_NU];
  const bool acc = rho > 0.0 && isfinite(cost_new);
  if (acc) {
    const double t = 2.0 * rho - 1.0;
    lam *= fmax(1.0 / 3.0, 1.0 - t * t * t);
    lam = fmin(fmax(lam, kPgLamMin), kPgLamMax);
    nu = 2.0;
    state[SLAM_BA_ST_CUR] = state[SLAM_BA_ST_CUR] != 0.0 ? 0.0 : 1.0;
    state[SLAM_BA_ST_COST] = cost_new;
    state[SLAM_BA_ST_NACCEPT] += 1.0;
  } else {
    lam = fmin(lam * nu, kPgLamMax);
    nu *= 2.0;
  }
  state[SLAM_BA_ST_LAMBDA] = lam;
  state[SLAM_BA_ST_NU] = nu;
  state[SLAM_BA_ST_COST_NEW] = cost_new;
  state[SLAM_BA_ST_PRED] = pred;
  state[SLAM_BA_ST_RHO] = rho;
  state[SLAM_BA_ST_ACCEPTED] = acc ? 1.0 : 0.0;
  state[SLAM_BA_ST_ITERS] += 1.0;
  state[SLAM_BA_ST_CHOL_FAIL] = fail ? 1.0 : 0.0;
}

__global__ void k_pg_reset(slam_pg_problem p, double lam0) {
  const int t = threadIdx.x;
  if (t < SLAM_BA_ST_SLOTS) p.state[t] = t == SLAM_BA_ST_LAMBDA ? lam0 : (t == SLAM_BA_ST_NU ? 2.0 : 0.0);
}

// ---------------------------------------------------------------- covariance
// Blocks of Sigma = H0^-1, H0 = J~^T J~ at the live poses with no
// damping: the factor of the LM step with k_pg_assemble<true>, a rank test of
// its pivots (k_pg_rank), then per distinct tile column c of the request the
// 64 columns X = Sigma E_c through the skyline factor, L Y = E_c forwards
// (k_pg_cov_fwd, tile rows c..T-1) and L^T X = Y backwards (k_pg_cov_bwd, tile
// rows T-1 down to the lowest one asked of that column), in the caller's
// workspace; all columns share every launch.  A block (a, b) is read from the
// column of the larger pose index (k_pg_cov_pick), the relative-pose
// covariance and the gate of a candidate edge from three of them (k_pg_gate).
struct PgCovLayout {  // inside d_ws: three int tables of T, then n_cols x T tiles (doubles)
  long long slot, low, col;  // ints: tile column -> slot or -1; its lowest tile row (T: none); slot -> tile column
  long long tiles, total;    // doubles
  __host__ __device__ PgCovLayout(int T, int n_cols) {
    slot = 0;
    low = T;
    col = 2ll * T;
    tiles = ((3ll * T + 1) / 2 + 7) / 8 * 8;
    total = tiles + (long long)n_cols * T * kTB * kTB;
  }
};

// The request's tables from the device copy of the list: entry (a, b) asks
// tile column max / 10 down to tile row min / 10 (gate: also both marginal
// blocks).  Slots in ascending column order; a column past n_cols (a device
// list that is not the host's) gets none, and its blocks come out NaN.
__global__ __launch_bounds__(kTlWG) void k_pg_cov_plan(int n_poses, int T, const int32_t* __restrict__ list,
                                                       int n, int gate, double* cws, int n_cols) {
  const PgCovLayout C(T, n_cols);
  int* tab = reinterpret_cast<int*>(cws);
  const int t = threadIdx.x;
  for (int q = t; q < T; q += kTlWG) {
    tab[C.slot + q] = -1;
    tab[C.low + q] = T;
    tab[C.col + q] = -1;
  }
  __syncthreads();
  for (int q = t; q < n; q += kTlWG) {
    const int a = list[2 * q], b = list[2 * q + 1];
    if ((unsigned)a >= (unsigned)n_poses || (unsigned)b >= (unsigned)n_poses) continue;
    const int ta = a / kPgTP, tb = b / kPgTP;
    atomicMin(tab + C.low + max(ta, tb), min(ta, tb));
    if (gate) atomicMin(tab + C.low + min(ta, tb), min(ta, tb));
  }
  __syncthreads();
  if (t >= 64) return;
  int run = 0;
  for (int base = 0; base < T; base += 64) {
    const int q = base + t;
    // (an agent-scope load: the minima were formed by atomics, past this CU's L1)
    const bool need = q < T && __hip_atomic_load(tab + C.low + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < T;
    const unsigned long long m = __ballot(need);
    const int s = run + __popcll(m & ((1ull << t) - 1ull));
    if (need && s < n_cols) {
      tab[C.slot + q] = s;
      tab[C.col + s] = q;
    }
    run += __popcll(m);
  }
}

// Every pivot against the stored diagonal: L_rr = 1 / (L_kk^-1)_rr from dinv,
// H_rr in D.  status[0] = 1 (and the failure flag raised for the kernels that
// follow) when the factor failed, a pivot is not finite or L_rr^2 <= rank_tol
// H_rr; words == 2: status[1] <- 0 for k_pg_gate's count.
__global__ __launch_bounds__(kTlWG) void k_pg_rank(PgArgs a, double rank_tol, int32_t* __restrict__ status,
                                                   int words) {
  const slam_pg_problem& p = a.p;
  const PgLayout L(p.n_poses, p.n_edges, a.T, a.n_tiles);
  __shared__ int okf;
  if (threadIdx.x == 0) okf = pg_failed(p.ws, L) ? 1 : 0;
  __syncthreads();
  bool bad = okf != 0;
  if (!bad) {
    for (int r = threadIdx.x; r < a.T * kTB; r += kTlWG) {
      const double xd = p.ws[L.dinv + (long long)(r >> 6) * kTB * kTB + (r & 63) * (kTB + 1)];
      const double piv = 1.0 / (xd * xd);
      bad = bad || !(xd > 0.0 && xd < INFINITY) || !(piv < INFINITY) || piv <= rank_tol * p.ws[L.d + r];
    }
  }
  const int any = __syncthreads_or(bad ? 1 : 0);
  if (threadIdx.x != 0) return;
  if (any) *reinterpret_cast<int*>(p.ws + L.flag) = 1;
  status[0] = any ? 1 : 0;
  if (words == 2) status[1] = 0;
}

// Forward, tile row k, one workgroup per requested column c (slot blockIdx.x;
// c > k: nothing yet): Y_c = L_cc^-1, Y_k = -L_kk^-1 sum_{J = max(first[k], c)}^{k-1} L_kJ Y_J.
__global__ __launch_bounds__(kTlWG) void k_pg_cov_fwd(PgArgs a, double* cws, int n_cols, int k) {
  const slam_pg_problem& p = a.p;
  const PgSched S(p.n_poses, p.n_edges, a.T, a.P);
  const PgLayout L(p.n_poses, p.n_edges, a.T, a.n_tiles);
  const PgCovLayout C(a.T, n_cols);
  __shared__ double Xf[kTB * kTB], Yf[kTB * kTB];
  __shared__ int okf;
  if (threadIdx.x == 0) okf = pg_failed(p.ws, L) ? 1 : 0;
  __syncthreads();
  if (okf != 0) return;
  const int c = reinterpret_cast<const int*>(cws)[C.col + blockIdx.x];
  if (c < 0 || c > k) return;
  double* X = cws + C.tiles + (long long)blockIdx.x * a.T * kTB * kTB;
  double* Yk = X + (long long)k * kTB * kTB;
  const double* Vkk = p.ws + L.dinv + (long long)k * kTB * kTB;
  if (k == c) {
    for (int e = threadIdx.x; e < kTB * kTB; e += kTlWG) Yk[e] = Vkk[e];
    return;
  }
  const int first = p.sched[S.first + k];
  const double* Lk = p.ws + L.tiles + (long long)(p.sched[S.rowoff + k] - first) * kTB * kTB;  // tile (k, 0)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  d4 acc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
  for (int J = max(first, c); J < k; ++J) {
    tile_to_frag(Lk + (long long)J * kTB * kTB, kTB, Xf);
    tile_to_frag_t(X + (long long)J * kTB * kTB, kTB, Yf);
    __syncthreads();
    tile_gemm_acc(Xf, Yf, acc);
    __syncthreads();  // Xf / Yf reloaded next J
  }
  tile_to_frag(Vkk, kTB, Xf);
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      Yf[frag_idx(s * 16 + (lane & 15), w * 16 + (lane >> 4) + 4 * r)] = acc[s][r];  // the sum, transposed image
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
  tile_gemm_acc(Xf, Yf, acc, true);
  tile_store(Yk, kTB, acc);
}

// Backward, tile row k, one workgroup per requested column (its lowest row >
// k: done): X_k = L_kk^-T (Y_k - sum_I L_Ik^T X_I), I over column k's panel
// rows, in place over Y_k (Y_k = 0 above the column's own tile row, unread).
__global__ __launch_bounds__(kTlWG) void k_pg_cov_bwd(PgArgs a, double* cws, int n_cols, int k) {
  const slam_pg_problem& p = a.p;
  const PgSched S(p.n_poses, p.n_edges, a.T, a.P);
  const PgLayout L(p.n_poses, p.n_edges, a.T, a.n_tiles);
  const PgCovLayout C(a.T, n_cols);
  __shared__ double Xf[kTB * kTB], Yf[kTB * kTB];
  __shared__ int okf;
  if (threadIdx.x == 0) okf = pg_failed(p.ws, L) ? 1 : 0;
  __syncthreads();
  if (okf != 0) return;
  const int* tab = reinterpret_cast<const int*>(cws);
  const int c = tab[C.col + blockIdx.x];
  if (c < 0 || tab[C.low + c] > k) return;
  const int32_t* first = p.sched + S.first;
  const int32_t* rowoff = p.sched + S.rowoff;
  const int r0 = p.sched[S.col_ptr + k], r1 = p.sched[S.col_ptr + k + 1];
  double* X = cws + C.tiles + (long long)blockIdx.x * a.T * kTB * kTB;
  double* Xk = X + (long long)k * kTB * kTB;
  const double* tiles = p.ws + L.tiles;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  d4 acc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
  for (int u = r0; u < r1; ++u) {
    const int I = p.sched[S.lists + u];
    tile_to_frag_t(tiles + (long long)(rowoff[I] + k - first[I]) * kTB * kTB, kTB, Xf);
    tile_to_frag_t(X + (long long)I * kTB * kTB, kTB, Yf);
    __syncthreads();
    tile_gemm_acc(Xf, Yf, acc);
    __syncthreads();  // Xf / Yf reloaded next I
  }
  tile_to_frag_t(p.ws + L.dinv + (long long)k * kTB * kTB, kTB, Xf);
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = w * 16 + (lane >> 4) + 4 * r, col = s * 16 + (lane & 15);
      const double y = k >= c ? Xk[row * kTB + col] : 0.0;
      Yf[frag_idx(col, row)] = y - acc[s][r];  // transposed image
    }
  __syncthreads();  // (every read of Y_k is done before the stores below)
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
  tile_gemm_acc(Xf, Yf, acc);
  tile_store(Xk, kTB, acc);
}

// Where Cov(a, b) lies: entry (m, n) = base[m * sr + n * sc], read from the
// column of the larger pose index (so block (a, b) is block (b, a) transposed
// bit for bit); base == nullptr: not in the request's tables.
struct PgBlk {
  const double* base;
  int sr, sc;
};
__device__ __forceinline__ PgBlk pg_cov_block(const double* cws, const PgCovLayout& C, int T, int n_cols, int a,
                                              int b) {
  const int* tab = reinterpret_cast<const int*>(cws);
  const int lo = min(a, b), hi = max(a, b);
  const int c = hi / kPgTP, r = lo / kPgTP;
  const int s = tab[C.slot + c];
  if (s < 0 || s >= n_cols || tab[C.low + c] > r) return PgBlk{nullptr, 0, 0};
  const double* tile = cws + C.tiles + ((long long)s * T + r) * kTB * kTB;
  const double* base = tile + (pg_row(lo) - r * kTB) * kTB + (pg_row(hi) - c * kTB);
  return a <= b ? PgBlk{base, kTB, 1} : PgBlk{base, 1, kTB};
}
__device__ __forceinline__ bool pg_held(const slam_pg_problem& p, int i, int q) {
  return p.pose_fixed != nullptr && ((p.pose_fixed[i] >> q) & 1u);
}
// Entry (m, n) of Cov(a, b): +0.0 on held rows and columns, the lower half
// mirrored when a == b.
__device__ __forceinline__ double pg_cov_entry(const slam_pg_problem& p, const PgBlk& B, int a, int b, int m,
                                               int n) {
  if (pg_held(p, a, m) || pg_held(p, b, n)) return 0.0;
  if (a == b) return B.base[max(m, n) * kTB + min(m, n)];
  return B.base[m * B.sr + n * B.sc];
}

// One workgroup per requested block: 36 lanes, one entry each.  NaN when the
// factor failed the rank test.
__global__ __launch_bounds__(64) void k_pg_cov_pick(PgArgs a, const int32_t* __restrict__ pairs,
                                                    const double* __restrict__ cws, int n_cols,
                                                    double* __restrict__ cov) {
  const slam_pg_problem& p = a.p;
  const PgLayout L(p.n_poses, p.n_edges, a.T, a.n_tiles);
  const PgCovLayout C(a.T, n_cols);
  __shared__ int okf;
  if (threadIdx.x == 0) okf = pg_failed(p.ws, L) ? 1 : 0;
  __syncthreads();
  const int t = threadIdx.x;
  if (t >= 36) return;
  const int i = pairs[2 * blockIdx.x], j = pairs[2 * blockIdx.x + 1];
  double v = __builtin_nan("");
  if (okf == 0 && (unsigned)i < (unsigned)p.n_poses && (unsigned)j < (unsigned)p.n_poses) {
    const PgBlk B = pg_cov_block(cws, C, a.T, n_cols, i, j);
    if (B.base != nullptr) v = pg_cov_entry(p, B, i, j, t / 6, t % 6);
  }
  cov[36ll * blockIdx.x + t] = v;
}

// Lower Cholesky of a symmetric 6x6 (full storage, lower half read and
// overwritten by L).  Pivot rule: bad when not finite or L_rr^2 <= tol * M_rr
// (tol = 0: not positive).
__device__ __forceinline__ bool pg_chol6(double M[36], double tol) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double mjj = M[7 * j];
    double d = mjj;
#pragma unroll
    for (int k = 0; k < j; ++k) d -= M[6 * j + k] * M[6 * j + k];
    ok = ok && d < INFINITY && d > tol * mjj && d > 0.0;
    const double l = sqrt(d), il = 1.0 / l;
    M[7 * j] = l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = M[6 * i + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= M[6 * i + k] * M[6 * j + k];
      M[6 * i + j] = s * il;
    }
  }
  return ok;
}
// y <- L^-1 y (lower L in full storage)
__device__ __forceinline__ void pg_fsub6(const double Lm[36], double y[6]) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = y[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= Lm[6 * i + k] * y[k];
    y[i] = s / Lm[7 * i];
  }
}

// G += f J1 Sigma_ab J2^T (6x6 row-major), Sigma_ab read entry by entry
__device__ __forceinline__ void pg_jsj(const slam_pg_problem& p, const PgBlk& B, int a, int b, const double J1[36],
                                       const double J2[36], double f, double G[36]) {
  double W[36];  // J1 Sigma_ab
#pragma unroll
  for (int m = 0; m < 36; ++m) W[m] = 0.0;
#pragma unroll
  for (int u = 0; u < 6; ++u)
#pragma unroll
    for (int v = 0; v < 6; ++v) {
      const double sg = pg_cov_entry(p, B, a, b, u, v);
#pragma unroll
      for (int m = 0; m < 6; ++m) W[6 * m + v] += J1[6 * m + u] * sg;
    }
#pragma unroll
  for (int m = 0; m < 6; ++m)
#pragma unroll
    for (int n = 0; n < 6; ++n) {
      double s = W[6 * m] * J2[6 * n];
#pragma unroll
      for (int v = 1; v < 6; ++v) s += W[6 * m + v] * J2[6 * n + v];
      G[6 * m + n] += f * s;
    }
}

// One lane per candidate edge k = (i, j, z_k, A_k), not required to be an edge
// of the graph: e, J_i, J_j as k_pg_lin forms them (nothing held, no weight),
// P = G + G^T with G = J_i S_ii J_i^T / 2 + J_i S_ij J_j^T + J_j S_jj J_j^T / 2
// (exactly symmetric), R = (A^T A)^-1 (0 without sqrt_info), S = P + R, d2 =
// e^T S^-1 e by a 6x6 Cholesky under the rank_tol rule; a candidate that fails
// it (or whose information is not positive definite) gets d2 = NaN and counts
// in status[1].  Every output NaN after a failed factor.
__global__ __launch_bounds__(kPgWG) void k_pg_gate(PgArgs a, const int32_t* __restrict__ cand,
                                                   const double* __restrict__ meas,
                                                   const double* __restrict__ sqrt_info, int n,
                                                   const double* __restrict__ cws, int n_cols, double rank_tol,
                                                   double* __restrict__ od2, double* __restrict__ oP,
                                                   double* __restrict__ oe, int32_t* __restrict__ status) {
  const slam_pg_problem& p = a.p;
  const PgLayout L(p.n_poses, p.n_edges, a.T, a.n_tiles);
  const PgCovLayout C(a.T, n_cols);
  __shared__ int okf;
  if (threadIdx.x == 0) okf = pg_failed(p.ws, L) ? 1 : 0;
  __syncthreads();
  const int k = blockIdx.x * kPgWG + threadIdx.x;
  if (k >= n) return;
  const double nan = __builtin_nan("");
  const int i = cand[2 * k], j = cand[2 * k + 1];
  PgBlk Bii{nullptr, 0, 0}, Bjj{nullptr, 0, 0}, Bij{nullptr, 0, 0};
  const bool in = (unsigned)i < (unsigned)p.n_poses && (unsigned)j < (unsigned)p.n_poses && i != j;
  if (okf == 0 && in) {
    Bii = pg_cov_block(cws, C, a.T, n_cols, i, i);
    Bjj = pg_cov_block(cws, C, a.T, n_cols, j, j);
    Bij = pg_cov_block(cws, C, a.T, n_cols, i, j);
  }
  if (Bii.base == nullptr || Bjj.base == nullptr || Bij.base == nullptr) {
    if (od2 != nullptr) od2[k] = nan;
    if (oP != nullptr)
      for (int m = 0; m < 36; ++m) oP[36ll * k + m] = nan;
    if (oe != nullptr)
      for (int m = 0; m < 6; ++m) oe[6ll * k + m] = nan;
    return;
  }
  const double* x = p.poses[pg_cur(p)];
  double xi[6], xj[6], z[6], e[6], Ji[36], Jj[36];
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    xi[q] = x[6 * i + q];
    xj[q] = x[6 * j + q];
    z[q] = meas[6ll * k + q];
  }
  pg_edge_raw<true>(xi, xj, z, 0u, 0u, e, Ji, Jj);
  double G[36];
#pragma unroll
  for (int m = 0; m < 36; ++m) G[m] = 0.0;
  pg_jsj(p, Bii, i, i, Ji, Ji, 0.5, G);
  pg_jsj(p, Bij, i, j, Ji, Jj, 1.0, G);
  pg_jsj(p, Bjj, j, j, Jj, Jj, 0.5, G);
  double Sm[36];
#pragma unroll
  for (int m = 0; m < 6; ++m)
#pragma unroll
    for (int q = 0; q <= m; ++q) Sm[6 * m + q] = Sm[6 * q + m] = G[6 * m + q] + G[6 * q + m];
  if (oe != nullptr)
#pragma unroll
    for (int m = 0; m < 6; ++m) oe[6ll * k + m] = e[m];
  if (oP != nullptr)
#pragma unroll
    for (int m = 0; m < 36; ++m) oP[36ll * k + m] = Sm[m];
  if (od2 == nullptr) return;
  bool ok = true;
  if (sqrt_info != nullptr) {
    // R = (A^T A)^-1 = M^-T M^-1, M the lower factor of A^T A: column q of M^-1 by a forward solve
    const double* A = sqrt_info + 36ll * k;
    double M[36];
#pragma unroll
    for (int m = 0; m < 6; ++m)
#pragma unroll
      for (int q = 0; q <= m; ++q) {
        double s = A[m] * A[q];
#pragma unroll
        for (int r = 1; r < 6; ++r) s += A[6 * r + m] * A[6 * r + q];
        M[6 * m + q] = M[6 * q + m] = s;
      }
    ok = pg_chol6(M, 0.0);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      double y[6];
#pragma unroll
      for (int m = 0; m < 6; ++m) y[m] = m == q ? 1.0 : 0.0;
      pg_fsub6(M, y);  // column q of M^-1 (zero above row q)
#pragma unroll
      for (int m = 0; m < 6; ++m) G[6 * m + q] = y[m];
    }
#pragma unroll
    for (int m = 0; m < 6; ++m)
#pragma unroll
      for (int q = 0; q <= m; ++q) {
        double s = 0.0;
#pragma unroll
        for (int r = m; r < 6; ++r) s += G[6 * r + m] * G[6 * r + q];
        Sm[6 * m + q] += s;
        if (q != m) Sm[6 * q + m] = Sm[6 * m + q];
      }
  }
  ok = pg_chol6(Sm, rank_tol) && ok;
  pg_fsub6(Sm, e);
  double d2 = e[0] * e[0];
#pragma unroll
  for (int q = 1; q < 6; ++q) d2 += e[q] * e[q];
  if (!ok) atomicAdd(status + 1, 1);
  od2[k] = ok ? d2 : nan;
}

// ---------------------------------------------------------------- host
// the edge list and the buffers every entry point reads
int pg_check_edges(const slam_pg_problem* p) {
  SLAM_REQUIRE(p != nullptr, "slam_pg: null problem");
  SLAM_REQUIRE(p->n_poses >= 1 && p->n_edges >= 1, "slam_pg: needs N >= 1 poses and E >= 1 edges, not %d, %d",
               p->n_poses, p->n_edges);
  SLAM_REQUIRE(p->n_poses <= (1 << 24) && p->n_edges <= (1 << 24), "slam_pg: more than 2^24 poses or edges");
  SLAM_REQUIRE(p->loss >= 0 && p->loss <= 3, "slam_pg: loss %d (0 linear, 1 huber, 2 soft_l1, 3 cauchy)", p->loss);
  SLAM_REQUIRE(p->loss == 0 || (std::isfinite(p->loss_scale) && p->loss_scale > 0.0),
               "slam_pg: loss %d needs a finite loss_scale > 0, not %g", p->loss, p->loss_scale);
  SLAM_REQUIRE(p->poses[0] && p->poses[1] && p->edge_ij && p->edge_ij_host && p->meas && p->sqrt_info,
               "slam_pg: null buffer");
  for (int k = 0; k < p->n_edges; ++k) {
    const int i = p->edge_ij_host[2 * k], j = p->edge_ij_host[2 * k + 1];
    SLAM_REQUIRE(i >= 0 && i < p->n_poses && j >= 0 && j < p->n_poses, "slam_pg: edge %d (%d, %d) out of range", k, i, j);
    SLAM_REQUIRE(i != j, "slam_pg: edge %d joins pose %d to itself", k, i);
  }
  return SLAM_OK;
}

// The host copy of the schedule against the edge list: every table the kernels
// index through is checked entry by entry, so a wrong one is refused rather
// than written through.
int pg_check(const slam_pg_problem* p, PgArgs* a) {
  if (int rc = pg_check_edges(p)) return rc;
  SLAM_REQUIRE(p->sched && p->sched_host && p->ws && p->state, "slam_pg: null buffer");
  const int N = p->n_poses, E = p->n_edges, T = (N + kPgTP - 1) / kPgTP;
  const int32_t* s = p->sched_host;
  SLAM_REQUIRE(p->sched_len >= kPgHdr, "slam_pg: schedule of %d ints", p->sched_len);
  SLAM_REQUIRE(s[0] == kPgMagic && s[1] == N && s[2] == E && s[3] == T,
               "slam_pg: schedule header (magic %#x, N %d, E %d, T %d) does not match the problem", s[0], s[1], s[2], s[3]);
  const int P = s[4];
  SLAM_REQUIRE(P >= 1 && P <= E, "slam_pg: schedule: %d pose pairs", P);
  const PgSched S(N, E, T, P);
  const long long n_rows = s[6], n_upd = s[7];
  SLAM_REQUIRE(n_rows >= 0 && n_upd >= 0 && S.lists + n_rows + 2 * n_upd == p->sched_len,
               "slam_pg: schedule length %d does not match its header", p->sched_len);
  const int32_t* first = s + S.first;
  const int32_t* rowoff = s + S.rowoff;
  SLAM_REQUIRE(rowoff[0] == 0, "slam_pg: schedule: rowoff[0]");
  for (int I = 0; I < T; ++I) {
    SLAM_REQUIRE(first[I] >= 0 && first[I] <= I, "slam_pg: schedule: first[%d] = %d", I, first[I]);
    SLAM_REQUIRE(rowoff[I + 1] == rowoff[I] + I - first[I] + 1, "slam_pg: schedule: rowoff[%d]", I + 1);
  }
  SLAM_REQUIRE(s[5] == rowoff[T], "slam_pg: schedule: stored tile count");
  // pose -> (edge, side), in edge order
  const int32_t* pp = s + S.pose_ptr;
  SLAM_REQUIRE(pp[0] == 0 && pp[N] == 2 * E, "slam_pg: schedule: pose_ptr ends");
  for (int i = 0; i < N; ++i) {
    SLAM_REQUIRE(pp[i + 1] >= pp[i] && pp[i + 1] <= 2 * E, "slam_pg: schedule: pose_ptr[%d]", i + 1);
    for (int q = pp[i]; q < pp[i + 1]; ++q) {
      const int en = s[S.pose_ent + q];
      SLAM_REQUIRE(en >= 0 && en < 2 * E && p->edge_ij_host[en] == i && (q == pp[i] || en > s[S.pose_ent + q - 1]),
                   "slam_pg: schedule: entry %d of pose %d", q, i);
    }
  }
  // unique pairs and their edges, in edge order
  const int32_t* qp = s + S.pair_ptr;
  SLAM_REQUIRE(qp[0] == 0 && qp[P] == E, "slam_pg: schedule: pair_ptr ends");
  for (int q = 0; q < P; ++q) {
    const int lo = s[S.pair_ij + 2 * q], hi = s[S.pair_ij + 2 * q + 1];
    SLAM_REQUIRE(lo >= 0 && lo < hi && hi < N, "slam_pg: schedule: pair %d (%d, %d)", q, lo, hi);
    SLAM_REQUIRE(q == 0 || s[S.pair_ij + 2 * q - 2] < lo || (s[S.pair_ij + 2 * q - 2] == lo && s[S.pair_ij + 2 * q - 1] < hi),
                 "slam_pg: schedule: pair %d out of order", q);
    SLAM_REQUIRE(qp[q + 1] > qp[q] && qp[q + 1] <= E, "slam_pg: schedule: pair_ptr[%d]", q + 1);
    SLAM_REQUIRE(first[hi / kPgTP] <= lo / kPgTP, "slam_pg: schedule: pair %d (%d, %d) lies outside the profile", q, lo, hi);
    for (int u = qp[q]; u < qp[q + 1]; ++u) {
      const int en = s[S.pair_ent + u];
      SLAM_REQUIRE(en >= 0 && en < 2 * E && (u == qp[q] || en > s[S.pair_ent + u - 1]),
                   "slam_pg: schedule: entry %d of pair %d", u, q);
      const int i = p->edge_ij_host[2 * (en >> 1)], j = p->edge_ij_host[2 * (en >> 1) + 1];
      SLAM_REQUIRE(std::min(i, j) == lo && std::max(i, j) == hi && (en & 1) == (i > j ? 1 : 0),
                   "slam_pg: schedule: entry %d of pair %d is edge (%d, %d)", u, q, i, j);
    }
  }
  // The column lists, in time linear in their length: column k's panel rows
  // are {I > k : first[I] <= k}; row I therefore sits in columns first[I]..I-1,
  // which a difference array turns into every column's count m_k.  A list of
  // m_k ascending rows that all qualify is that set.
  const int32_t* cp = s + S.col_ptr;
  const int32_t* upp = s + S.upd_ptr;
  SLAM_REQUIRE(cp[0] == 0 && upp[0] == 0, "slam_pg: schedule: list starts");
  int max_rows = 0, max_upd = 0;
  std::vector<int> cnt(T + 1, 0);
  for (int I = 0; I < T; ++I) {
    cnt[first[I]] += 1;
    cnt[I] -= 1;
  }
  int m = 0;
  for (int k = 0; k < T; ++k) {
    m += cnt[k];
    const long long mu = (long long)m * (m + 1) / 2;
    SLAM_REQUIRE(cp[k + 1] == cp[k] + m && cp[k + 1] <= n_rows, "slam_pg: schedule: col_ptr[%d]", k + 1);
    SLAM_REQUIRE(upp[k + 1] == upp[k] + mu && upp[k + 1] <= n_upd, "slam_pg: schedule: upd_ptr[%d]", k + 1);
    const int32_t* rk = s + S.lists + cp[k];
    const int32_t* up = s + S.lists + n_rows + 2ll * upp[k];
    int u = 0;
    for (int x = 0; x < m; ++x) {
      const int I = rk[x];
      SLAM_REQUIRE(I > k && I < T && first[I] <= k && (x == 0 || I > rk[x - 1]),
                   "slam_pg: schedule: panel row %d of column %d", x, k);
      for (int y = 0; y <= x; ++y, ++u)
        SLAM_REQUIRE(up[2 * u] == I && up[2 * u + 1] == rk[y], "slam_pg: schedule: update pair %d of column %d", u, k);
    }
    max_rows = std::max(max_rows, m);
    max_upd = std::max(max_upd, (int)mu);
  }
  SLAM_REQUIRE(cp[T] == n_rows && upp[T] == n_upd, "slam_pg: schedule: list totals");
  SLAM_REQUIRE(s[8] == max_rows && s[9] == max_upd, "slam_pg: schedule: list maxima");
  const long long need = PgLayout(N, E, T, rowoff[T]).total;
  if (p->ws_len < need) {
    slam::set_error("slam_pg: workspace of %lld doubles, needs %lld", p->ws_len, need);
    return SLAM_ERR_WORKSPACE;
  }
  a->p = *p;
  a->T = T;
  a->P = P;
  a->n_tiles = rowoff[T];
  return SLAM_OK;
}

// Linearise, assemble (COV: undamped, for the covariance) and factor: the
// column sweep of the skyline Cholesky.
template <bool COV>
int pg_launch_factor(const PgArgs& a, hipStream_t s) {
  const slam_pg_problem& p = a.p;
  const PgSched S(p.n_poses, p.n_edges, a.T, a.P);
  const PgLayout L(p.n_poses, p.n_edges, a.T, a.n_tiles);
  const int32_t* cp = p.sched_host + S.col_ptr;
  const int32_t* up = p.sched_host + S.upd_ptr;
  double* rec = p.ws + L.rec;
  k_pg_lin<true><<<nblk(p.n_edges, kPgWG), kPgWG, 0, s>>>(p, nullptr, 0, rec, kPgRec, rec + 6, rec + 42, kPgRec);
  SLAM_LAUNCHED("k_pg_lin");
  k_pg_zero<<<(int)a.n_tiles, kTlWG, 0, s>>>(a);
  SLAM_LAUNCHED("k_pg_zero");
  k_pg_assemble<COV><<<p.n_poses + a.P, kPgWG, 0, s>>>(a);
  SLAM_LAUNCHED("k_pg_assemble");
  for (int k = 0; k < a.T; ++k) {
    k_pg_panel<<<1 + cp[k + 1] - cp[k], kTlWG, 0, s>>>(a, k);
    SLAM_LAUNCHED("k_pg_panel");
    if (up[k + 1] > up[k]) {
      k_pg_update<<<up[k + 1] - up[k], kTlWG, 0, s>>>(a, k);
      SLAM_LAUNCHED("k_pg_update");
    }
  }
  return SLAM_OK;
}

// The launch geometry of a covariance request, from the host copy of its list
// (k_pg_cov_plan builds the same tables on the device): the distinct tile
// columns, the first one, and the lowest tile row any of them is asked for.
struct PgCovGeom {
  int n_cols, c_min, r_min;
};

// What slam_pg_covariance and slam_pg_gate refuse, in one place; `gate`: the
// list holds candidate edges (i != j, both marginal blocks needed too).
int pg_cov_check(const char* who, const slam_pg_problem* prob, const int32_t* d_list, const int32_t* list_host,
                 int n, bool gate, double rank_tol, const double* d_ws, long long ws_len, const int32_t* d_status,
                 PgArgs* a, PgCovGeom* g) {
  if (int rc = pg_check(prob, a)) return rc;
  SLAM_REQUIRE(d_list != nullptr && list_host != nullptr && d_ws != nullptr && d_status != nullptr,
               "%s: null pointer", who);
  SLAM_REQUIRE(n >= 1, "%s: count %d < 1", who, n);
  SLAM_REQUIRE(std::isfinite(rank_tol) && rank_tol >= 0.0 && rank_tol < 1.0,
               "%s: rank_tol %g must be finite and in [0, 1)", who, rank_tol);
  const int N = prob->n_poses, T = a->T;
  std::vector<int> low(T, T);
  for (int q = 0; q < n; ++q) {
    const int i = list_host[2 * q], j = list_host[2 * q + 1];
    SLAM_REQUIRE(i >= 0 && i < N && j >= 0 && j < N, "%s: entry %d (%d, %d) out of range", who, q, i, j);
    SLAM_REQUIRE(!gate || i != j, "%s: candidate %d joins pose %d to itself", who, q, i);
    const int ti = i / kPgTP, tj = j / kPgTP;
    low[std::max(ti, tj)] = std::min(low[std::max(ti, tj)], std::min(ti, tj));
    if (gate) low[std::min(ti, tj)] = std::min(low[std::min(ti, tj)], std::min(ti, tj));
  }
  g->n_cols = 0;
  g->c_min = g->r_min = T;
  for (int c = 0; c < T; ++c)
    if (low[c] < T) {
      g->n_cols += 1;
      g->c_min = std::min(g->c_min, c);
      g->r_min = std::min(g->r_min, low[c]);
    }
  const long long need = PgCovLayout(T, g->n_cols).total;
  if (ws_len < need) {
    slam::set_error("%s: workspace of %lld doubles, slam_pg_cov_workspace_len(%d, %d) gives %lld", who, ws_len, N,
                    g->n_cols, need);
    return SLAM_ERR_WORKSPACE;
  }
  return SLAM_OK;
}

// The factor of H0 (the LM step's launches with k_pg_assemble<true>), the
// request's tables, the rank test, and both sweeps: the factor's launches + 2 +
// at most 2 T, whatever the request.
int pg_cov_launch(const PgArgs& a, const PgCovGeom& g, const int32_t* d_list, int n, bool gate, double rank_tol,
                  double* d_ws, int32_t* d_status, hipStream_t s) {
  if (int rc = pg_launch_factor<true>(a, s)) return rc;
  k_pg_cov_plan<<<1, kTlWG, 0, s>>>(a.p.n_poses, a.T, d_list, n, gate ? 1 : 0, d_ws, g.n_cols);
  SLAM_LAUNCHED("k_pg_cov_plan");
  k_pg_rank<<<1, kTlWG, 0, s>>>(a, rank_tol, d_status, gate ? 2 : 1);
  SLAM_LAUNCHED("k_pg_rank");
  for (int k = g.c_min; k < a.T; ++k) {
    k_pg_cov_fwd<<<g.n_cols, kTlWG, 0, s>>>(a, d_ws, g.n_cols, k);
    SLAM_LAUNCHED("k_pg_cov_fwd");
  }
  for (int k = a.T - 1; k >= g.r_min; --k) {
    k_pg_cov_bwd<<<g.n_cols, kTlWG, 0, s>>>(a, d_ws, g.n_cols, k);
    SLAM_LAUNCHED("k_pg_cov_bwd");
  }
  return SLAM_OK;
}

}  // namespace

extern "C" int slam_pg_problem_size(void) { return (int)sizeof(slam_pg_problem); }

extern "C" long long slam_pg_workspace_len(int n_poses, int n_edges, int n_tiles_stored) {
  if (n_poses < 1 || n_edges < 1 || n_tiles_stored < 1) {
    slam::set_error("slam_pg_workspace_len: bad sizes %d, %d, %d", n_poses, n_edges, n_tiles_stored);
    return SLAM_ERR_ARG;
  }
  return PgLayout(n_poses, n_edges, (n_poses + kPgTP - 1) / kPgTP, n_tiles_stored).total;
}

extern "C" int slam_pg_reset(const slam_pg_problem* prob, double lambda0, void* stream) {
  PgArgs a;
  if (int rc = pg_check(prob, &a)) return rc;
  SLAM_REQUIRE(std::isfinite(lambda0) && lambda0 > 0.0, "slam_pg_reset: lambda0 %g", lambda0);
  hipStream_t s = slam::as_stream(stream);
  k_pg_reset<<<1, 64, 0, s>>>(a.p, lambda0);
  SLAM_LAUNCHED("k_pg_reset");
  k_pg_trial<<<nblk(a.p.n_edges, kPgWG), kPgWG, 0, s>>>(a, 0);
  SLAM_LAUNCHED("k_pg_trial");
  k_pg_decide<<<1, kPgSumWG, 0, s>>>(a, 0);
  SLAM_LAUNCHED("k_pg_decide");
  return SLAM_OK;
}

extern "C" int slam_pg_iterate(const slam_pg_problem* prob, int n_iters, void* stream) {
  PgArgs a;
  if (int rc = pg_check(prob, &a)) return rc;
  SLAM_REQUIRE(n_iters >= 0, "slam_pg_iterate: n_iters %d", n_iters);
  hipStream_t s = slam::as_stream(stream);
  const slam_pg_problem& p = a.p;
  for (int it = 0; it < n_iters; ++it) {
    if (int rc = pg_launch_factor<false>(a, s)) return rc;
    for (int k = a.T - 1; k >= 0; --k) {
      k_pg_back<<<1, kTlWG, 0, s>>>(a, k);
      SLAM_LAUNCHED("k_pg_back");
    }
    k_pg_trial<<<nblk(std::max(p.n_edges, 6 * p.n_poses), kPgWG), kPgWG, 0, s>>>(a, 1);
    SLAM_LAUNCHED("k_pg_trial");
    k_pg_decide<<<1, kPgSumWG, 0, s>>>(a, 1);
    SLAM_LAUNCHED("k_pg_decide");
  }
  return SLAM_OK;
}

extern "C" int slam_pg_residual(const slam_pg_problem* prob, double* d_e, double* d_r, void* stream) {
  if (int rc = pg_check_edges(prob)) return rc;
  SLAM_REQUIRE(d_e != nullptr || d_r != nullptr, "slam_pg_residual: null outputs");
  k_pg_lin<false><<<nblk(prob->n_edges, kPgWG), kPgWG, 0, slam::as_stream(stream)>>>(
      *prob, d_e, 6, d_r, 6, nullptr, nullptr, 0);
  SLAM_LAUNCHED("k_pg_lin");
  return SLAM_OK;
}

extern "C" int slam_pg_jacobian(const slam_pg_problem* prob, double* d_Ji, double* d_Jj, void* stream) {
  if (int rc = pg_check_edges(prob)) return rc;
  SLAM_REQUIRE(d_Ji != nullptr && d_Jj != nullptr, "slam_pg_jacobian: null outputs");
  k_pg_lin<true><<<nblk(prob->n_edges, kPgWG), kPgWG, 0, slam::as_stream(stream)>>>(
      *prob, nullptr, 0, nullptr, 0, d_Ji, d_Jj, 36);
  SLAM_LAUNCHED("k_pg_lin");
  return SLAM_OK;
}

extern "C" long long slam_pg_cov_workspace_len(int n_poses, int n_cols) {
  const int T = n_poses >= 1 && n_poses <= (1 << 24) ? (n_poses + kPgTP - 1) / kPgTP : 0;  // 0: refused below
  if (n_cols < 1 || n_cols > T) {
    slam::set_error("slam_pg_cov_workspace_len: bad sizes %d poses, %d tile columns", n_poses, n_cols);
    return SLAM_ERR_ARG;
  }
  return PgCovLayout(T, n_cols).total;
}

extern "C" int slam_pg_covariance(const slam_pg_problem* prob, const int32_t* d_pairs, const int32_t* pairs_host,
                                  int n_pairs, double rank_tol, double* d_cov, double* d_ws, long long ws_len,
                                  int32_t* d_status, void* stream) {
  PgArgs a;
  PgCovGeom g;
  if (int rc = pg_cov_check("slam_pg_covariance", prob, d_pairs, pairs_host, n_pairs, false, rank_tol, d_ws, ws_len,
                            d_status, &a, &g))
    return rc;
  SLAM_REQUIRE(d_cov != nullptr, "slam_pg_covariance: null pointer");
  hipStream_t s = slam::as_stream(stream);
  if (int rc = pg_cov_launch(a, g, d_pairs, n_pairs, false, rank_tol, d_ws, d_status, s)) return rc;
  k_pg_cov_pick<<<n_pairs, 64, 0, s>>>(a, d_pairs, d_ws, g.n_cols, d_cov);
  SLAM_LAUNCHED("k_pg_cov_pick");
  return SLAM_OK;
}

extern "C" int slam_pg_gate(const slam_pg_problem* prob, const int32_t* d_cand_ij, const int32_t* cand_ij_host,
                            const double* d_meas, const double* d_sqrt_info, int n_cand, double rank_tol,
                            double* d_d2, double* d_P, double* d_e, double* d_ws, long long ws_len,
                            int32_t* d_status, void* stream) {
  PgArgs a;
  PgCovGeom g;
  if (int rc = pg_cov_check("slam_pg_gate", prob, d_cand_ij, cand_ij_host, n_cand, true, rank_tol, d_ws, ws_len,
                            d_status, &a, &g))
    return rc;
  SLAM_REQUIRE(d_meas != nullptr, "slam_pg_gate: null pointer");
  SLAM_REQUIRE(d_d2 != nullptr || d_P != nullptr || d_e != nullptr, "slam_pg_gate: null outputs");
  hipStream_t s = slam::as_stream(stream);
  if (int rc = pg_cov_launch(a, g, d_cand_ij, n_cand, true, rank_tol, d_ws, d_status, s)) return rc;
  k_pg_gate<<<nblk(n_cand, kPgWG), kPgWG, 0, s>>>(a, d_cand_ij, d_meas, d_sqrt_info, n_cand, d_ws, g.n_cols,
                                                  rank_tol, d_d2, d_P, d_e, d_status);
  SLAM_LAUNCHED("k_pg_gate");
  return SLAM_OK;
}
