// Structure-only refinement of the landmarks from their track rows: the poses
// are held and every landmark is refined from all of its observations in a
// window of frames -- the counterpart of pose_refine.hip.  slam_points_refine
// in include/slam355.h states the definition; this file is its two kernels.
//
//   k_points_index   one lane per track row: the row's k races into the index
//                    word [frame][landmark] of the workspace (integer
//                    atomicMin, as k_spawn_claim: the lowest k of a frame wins
//                    whatever the arrival order) and the row's mask byte is
//                    cleared.  The frame-major rows become landmark-major reads
//                    without a sort;
//   k_points_refine  one lane per landmark: consecutive lanes read consecutive
//                    index words (the pattern of k_map_score), the window's
//                    poses (12 doubles per frame) are staged once per workgroup
//                    in LDS, the active set and the inlier set are 64-bit
//                    register masks, and the 3x3 sums, the Cholesky and the
//                    decision run in the lane's f64 registers in frame order: a
//                    lane is a sequential evaluation of the header's text.  A
//                    landmark is a chain of n_rounds * iters dependent LM
//                    iterations over a handful of observations; with tens of
//                    thousands of landmarks the lanes are the parallelism and
//                    no sum ever crosses a lane.  The lane gathers its pixels
//                    once (one pass over the frames, the loads of eight frames
//                    in flight) into a compact list in LDS, its first kObsLds
//                    observations in frame order; every later pass walks the
//                    set bits of its frame mask and reads the list, so a pass
//                    costs the observations a wave's landmarks have, not the
//                    frames of the window times two dependent global loads (the
//                    first shape: profiles/points_refine/).  Observations
//                    beyond kObsLds are read through the index again.
// Nothing here waits for another workgroup: the index goes from the first
// launch to the second through memory and the launch boundary.
#include "common.hpp"
#include "pose_math.hpp"
#include "robust_loss.hpp"

namespace {

constexpr int kWG = 256;    // k_points_index
constexpr int kLanes = 128;  // k_points_refine: landmarks per workgroup
constexpr int kMaxFrames = 64;     // the active set is one 64-bit mask
constexpr int kObsLds = 16;  // observations per landmark kept in LDS (16 B each)
constexpr int kPose = 13;    // doubles per staged pose: 12 and one of padding (lanes read different frames)
constexpr int kNoRow = 0x7f7f7f7f;  // an index word after the memset: above every k

struct PointsArgs {
  const double* rows;
  const int32_t* count;
  const double* poses;
  const double* P;
  double* X;
  const int32_t* n;
  int32_t* tab;  // workspace: [n_frames][x_cap] lowest row of the frame that names the landmark
  int32_t* status;
  int32_t* nobs;
  double* cost;
  double* info;
  double* var;
  uint8_t* mask;
  int32_t* nkilled;
  int n_frames, rows_cap, x_cap, loss, n_rounds, iters, min_obs, kill;
  double loss_scale, gate, min_depth, max_var;
};

__global__ __launch_bounds__(kWG) void k_points_index(const PointsArgs a) {
  const int f = blockIdx.y, k = blockIdx.x * kWG + threadIdx.x;
  const int cnt = min(max(a.count[f], 0), a.rows_cap);
  if (k >= cnt) return;
  const size_t row = (size_t)f * a.rows_cap + k;
  a.mask[row] = 0;
  const double l = a.rows[4 * row + 1];
  if (!(l >= 0.0 && l < (double)a.x_cap)) return;  // NaN: nobody's
  const int i = (int)l;                            // 0 <= i < x_cap
  if ((double)i == l) atomicMin(&a.tab[(size_t)f * a.x_cap + i], k);
}

// Residual of the pixel (x, y) of a frame with pose T (12 doubles: the first
// three rows of the camera-to-world matrix) at the world point X, optionally
// the 2x3 Jacobian wrt X; returns whether the observation is valid at X.
template <bool JAC>
__device__ __forceinline__ bool point_residual(const double* T, const double* P, const double X[3],
                                               double x, double y, double min_depth, double r[2],
                                               double J[2][3]) {
  const double d0 = X[0] - T[3], d1 = X[1] - T[7], d2 = X[2] - T[11];
  double Xc[3], uv[2], a[2][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) Xc[k] = T[k] * d0 + T[4 + k] * d1 + T[8 + k] * d2;
  const double h2 = P[8] * Xc[0] + P[9] * Xc[1] + P[10] * Xc[2] + P[11];
  vo_project<JAC>(P, Xc, uv, a);
  r[0] = uv[0] - x;
  r[1] = uv[1] - y;
  if constexpr (JAC) {
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        J[c][k] = a[c][0] * T[4 * k] + a[c][1] * T[4 * k + 1] + a[c][2] * T[4 * k + 2];
  }
  return Xc[2] > min_depth && h2 > 0.0;
}

// Solve (H + lam max(diag H, 1e-12)) d = -g for the 3x3 system, H as its lower
// triangle (00 10 11 20 21 22); solve6 of pose_math.hpp at size 3.
__device__ __forceinline__ bool solve3(const double H[6], const double g[3], double lam,
                                       double d[3]) {
  const double a00 = H[0] + lam * fmax(H[0], 1e-12);
  const double a11 = H[2] + lam * fmax(H[2], 1e-12);
  const double a22 = H[5] + lam * fmax(H[5], 1e-12);
  if (!(a00 > 0.0)) return false;
  const double l00 = sqrt(a00);
  const double l10 = H[1] / l00, l20 = H[3] / l00;
  const double s1 = a11 - l10 * l10;
  if (!(s1 > 0.0)) return false;
  const double l11 = sqrt(s1);
  const double l21 = (H[4] - l20 * l10) / l11;
  const double s2 = (a22 - l20 * l20) - l21 * l21;
  if (!(s2 > 0.0)) return false;
  const double l22 = sqrt(s2);
  const double y0 = -g[0] / l00;
  const double y1 = (-g[1] - l10 * y0) / l11;
  const double y2 = ((-g[2] - l20 * y0) - l21 * y1) / l22;
  d[2] = y2 / l22;
  d[1] = (y1 - l21 * d[2]) / l11;
  d[0] = ((y0 - l10 * d[1]) - l20 * d[2]) / l00;
  return true;
}

// The largest diagonal entry of H^-1 through the Cholesky factor of the
// undamped H; false when a pivot is not positive and finite.
__device__ __forceinline__ bool max_variance(const double H[6], double& var) {
  const double inf = __builtin_inf();
  if (!(H[0] > 0.0 && H[0] < inf)) return false;
  const double l00 = sqrt(H[0]);
  const double l10 = H[1] / l00, l20 = H[3] / l00;
  const double s1 = H[2] - l10 * l10;
  if (!(s1 > 0.0 && s1 < inf)) return false;
  const double l11 = sqrt(s1);
  const double l21 = (H[4] - l20 * l10) / l11;
  const double s2 = (H[5] - l20 * l20) - l21 * l21;
  if (!(s2 > 0.0 && s2 < inf)) return false;
  const double l22 = sqrt(s2);
  // M = L^-1, H^-1 = M^T M
  const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
  const double m10 = -(l10 * m00) / l11;
  const double m21 = -(l21 * m11) / l22;
  const double m20 = -(l20 * m00 + l21 * m10) / l22;
  const double v0 = (m00 * m00 + m10 * m10) + m20 * m20;
  const double v1 = m11 * m11 + m21 * m21;
  const double v2 = m22 * m22;
  var = fmax(v0, fmax(v1, v2));
  return true;
}

__global__ __launch_bounds__(kLanes) void k_points_refine(const PointsArgs a) {
  __shared__ double sT[kMaxFrames * kPose];
  __shared__ double2 sObs[kObsLds][kLanes];  // [j][lane]: consecutive lanes, consecutive 16 bytes
  const int t = threadIdx.x, nf = a.n_frames;
  for (int j = t; j < nf * 12; j += kLanes)
    sT[kPose * (j / 12) + j % 12] = a.poses[16 * (size_t)(j / 12) + j % 12];
  __syncthreads();
  const long long li = (long long)blockIdx.x * kLanes + t;
  if (li >= a.x_cap) return;
  const int i = (int)li;
  double* info = a.info + 9 * (size_t)i;
  auto nothing = [&](int status) {  // the outputs of a landmark that is not optimised
    a.status[i] = status;
    a.nobs[i] = -1;
    a.cost[i] = 0.0;
    a.var[i] = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) info[k] = 0.0;
  };
  if (i >= min(max(*a.n, 0), a.x_cap)) return nothing(-1);
  double* Xp = a.X + 3 * (size_t)i;
  const double Xin[3] = {Xp[0], Xp[1], Xp[2]};
  if (Xin[0] != Xin[0]) return nothing(4);  // dead: its rows keep the 0 of k_points_index
  double P[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = a.P[k];
  const double gate2 = a.gate * a.gate;
  const int loss = a.loss, rows_cap = a.rows_cap;
  const int32_t* tab = a.tab + i;
  const size_t x_cap = (size_t)a.x_cap;
  auto pixel = [&](int fr, int k) {  // (x, y) of row k of frame fr; d_rows is 8-byte aligned only
    const double* rw = a.rows + 4 * ((size_t)fr * rows_cap + k);
    return make_double2(rw[2], rw[3]);
  };

  // the frames that observe the landmark; their pixels, in frame order, into the list
  unsigned long long has = 0ull;
#pragma unroll 8
  for (int fr = 0; fr < nf; ++fr) {
    const int k = tab[fr * x_cap];
    const bool obs = k < rows_cap;  // kNoRow otherwise
    const double2 xy = pixel(fr, obs ? k : 0);
    const int j = __popcll(has);
    if (obs && j < kObsLds) sObs[j][t] = xy;
    has |= obs ? 1ull << fr : 0ull;
  }
  // f(frame, x, y) for the frames of `set` (a subset of `has`), ascending
  auto for_obs = [&](unsigned long long set, auto&& f) {
    unsigned long long rem = has;
    for (int j = 0; rem != 0ull; ++j) {
      const int fr = __ffsll((long long)rem) - 1;
      rem &= rem - 1ull;
      if (!((set >> fr) & 1ull)) continue;
      double2 xy;
      if (j < kObsLds)
        xy = sObs[j][t];
      else
        xy = pixel(fr, tab[fr * x_cap]);
      f(fr, xy.x, xy.y);
    }
  };
  // those valid at the input point
  unsigned long long act = 0ull;
  for_obs(has, [&](int fr, double x, double y) {
    double r[2], J[2][3];
    if (point_residual<false>(sT + kPose * fr, P, Xin, x, y, a.min_depth, r, J)) act |= 1ull << fr;
  });
  auto write_mask = [&](unsigned long long set) {
    for_obs(set, [&](int fr, double, double) {
      a.mask[(size_t)fr * rows_cap + tab[fr * x_cap]] = 1;
    });
  };
  if (__popcll(act) < a.min_obs) {
    write_mask(act);
    return nothing(1);
  }
  // H (lower triangle), g and the cost over `set` at X
  auto normal_sums = [&](unsigned long long set, const double X[3], double H[6], double g[3],
                         double& cost) {
#pragma unroll
    for (int k = 0; k < 6; ++k) H[k] = 0.0;
    g[0] = g[1] = g[2] = 0.0;
    cost = 0.0;
    for_obs(set, [&](int fr, double x, double y) {
      double r[2], J[2][3];
      point_residual<true>(sT + kPose * fr, P, X, x, y, a.min_depth, r, J);
      const double term = loss != 0 ? robust_weight<3>(r, J[0], J[1], loss, a.loss_scale)
                                    : r[0] * r[0] + r[1] * r[1];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        int k = 0;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
#pragma unroll
          for (int v = 0; v <= u; ++v) H[k++] += J[c][u] * J[c][v];
          g[u] += J[c][u] * r[c];
        }
      }
      cost += term;
    });
  };

  double X[3] = {Xin[0], Xin[1], Xin[2]};
  int status = 0;
  for (int round = 0; round < a.n_rounds && status == 0; ++round) {
    double lam = 1e-3;
    for (int it = 0; it < a.iters; ++it) {
      double H[6], g[3], cost, d[3];
      normal_sums(act, X, H, g, cost);
      bool ok = solve3(H, g, lam, d);
      if (ok) {
        const double Xn[3] = {X[0] + d[0], X[1] + d[1], X[2] + d[2]};
        double cn = 0.0;
        for_obs(act, [&](int fr, double x, double y) {
          double r[2], J[2][3];
          if (!point_residual<false>(sT + kPose * fr, P, Xn, x, y, a.min_depth, r, J)) ok = false;
          cn += loss != 0 ? robust_weight<0>(r, nullptr, nullptr, loss, a.loss_scale)
                          : r[0] * r[0] + r[1] * r[1];
        });
        ok = ok && cn < cost;
        if (ok) {
          X[0] = Xn[0];
          X[1] = Xn[1];
          X[2] = Xn[2];
        }
      }
      lam = ok ? fmax(lam * 0.1, 1e-12) : fmin(lam * 10.0, 1e12);
    }
    // every observation of the landmark, not only those of the active set
    act = 0ull;
    for_obs(has, [&](int fr, double x, double y) {
      double r[2], J[2][3];
      const bool v = point_residual<false>(sT + kPose * fr, P, X, x, y, a.min_depth, r, J);
      if (v && r[0] * r[0] + r[1] * r[1] <= gate2) act |= 1ull << fr;
    });
    if (__popcll(act) < a.min_obs) status = 2;
  }
  write_mask(act);
  if (status != 0) {
    nothing(2);
    if (a.kill) {
      const double nan = __builtin_nan("");
      Xp[0] = nan;
      Xp[1] = nan;
      Xp[2] = nan;
      atomicAdd(a.nkilled, 1);  // one add per wave after the compiler's lane count
    }
    return;
  }
  double H[6], g[3], cost, var = __builtin_inf();
  normal_sums(act, X, H, g, cost);
  const bool pd = max_variance(H, var);
  if (!pd) var = __builtin_inf();
  status = pd && var <= a.max_var ? 0 : 3;
  if (status == 0) {
    Xp[0] = X[0];
    Xp[1] = X[1];
    Xp[2] = X[2];
  }
  a.status[i] = status;
  a.nobs[i] = __popcll(act);
  a.cost[i] = cost;
  a.var[i] = var;
  info[0] = H[0]; info[1] = H[1]; info[2] = H[3];
  info[3] = H[1]; info[4] = H[2]; info[5] = H[4];
  info[6] = H[3]; info[7] = H[4]; info[8] = H[5];
}

size_t points_ws_bytes(int n_frames, int x_cap) {
  return (size_t)n_frames * (size_t)x_cap * sizeof(int32_t);
}

}  // namespace

extern "C" int slam_points_refine_workspace_bytes(int n_frames, int x_cap, size_t* bytes) {
  SLAM_REQUIRE(n_frames >= 1 && n_frames <= kMaxFrames,
               "slam_points_refine_workspace_bytes: n_frames %d not in 1..%d", n_frames, kMaxFrames);
  SLAM_REQUIRE(x_cap >= 1, "slam_points_refine_workspace_bytes: x_cap %d < 1", x_cap);
  NEED("slam_points_refine_workspace_bytes", bytes);
  *bytes = points_ws_bytes(n_frames, x_cap);
  return SLAM_OK;
}

extern "C" int slam_points_refine(const double* d_rows, const int32_t* d_count, int rows_cap,
                                  int n_frames, const double* d_poses, const double* d_P,
                                  double* d_X, const int32_t* d_n, int x_cap, int loss,
                                  double loss_scale, double gate, double min_depth, int n_rounds,
                                  int iters, int min_obs, double max_var, int kill,
                                  int32_t* d_status, int32_t* d_nobs, double* d_cost,
                                  double* d_info, double* d_var, uint8_t* d_mask,
                                  int32_t* d_nkilled, void* d_ws, size_t ws_bytes, void* stream) {
  NEED("slam_points_refine", d_rows);
  NEED("slam_points_refine", d_count);
  NEED("slam_points_refine", d_poses);
  NEED("slam_points_refine", d_P);
  NEED("slam_points_refine", d_X);
  NEED("slam_points_refine", d_n);
  NEED("slam_points_refine", d_status);
  NEED("slam_points_refine", d_nobs);
  NEED("slam_points_refine", d_cost);
  NEED("slam_points_refine", d_info);
  NEED("slam_points_refine", d_var);
  NEED("slam_points_refine", d_mask);
  NEED("slam_points_refine", d_nkilled);
  NEED("slam_points_refine", d_ws);
  SLAM_REQUIRE(n_frames >= 1 && n_frames <= kMaxFrames, "slam_points_refine: n_frames %d not in 1..%d",
               n_frames, kMaxFrames);
  SLAM_REQUIRE(rows_cap >= 1 && rows_cap <= 65535, "slam_points_refine: rows_cap %d not in 1..65535",
               rows_cap);
  SLAM_REQUIRE(x_cap >= 1, "slam_points_refine: x_cap %d < 1", x_cap);
  SLAM_REQUIRE(n_rounds >= 1 && n_rounds <= 8, "slam_points_refine: n_rounds %d not in 1..8",
               n_rounds);
  SLAM_REQUIRE(iters >= 1 && iters <= 50, "slam_points_refine: iters %d not in 1..50", iters);
  SLAM_REQUIRE(min_obs >= 2, "slam_points_refine: min_obs %d < 2", min_obs);
  SLAM_REQUIRE(loss >= 0 && loss <= 3, "slam_points_refine: loss %d not in 0..3", loss);
  SLAM_REQUIRE(loss == 0 || loss_scale > 0.0, "slam_points_refine: loss_scale must be > 0");
  SLAM_REQUIRE(gate > 0.0, "slam_points_refine: gate must be > 0");  // NaN refused too
  SLAM_REQUIRE(min_depth == min_depth, "slam_points_refine: min_depth is NaN");
  SLAM_REQUIRE(max_var > 0.0, "slam_points_refine: max_var must be > 0 (+inf: no bound)");
  SLAM_REQUIRE(((uintptr_t)d_ws & 3) == 0, "slam_points_refine: d_ws must be 4-byte aligned");
  SLAM_REQUIRE(ws_bytes >= points_ws_bytes(n_frames, x_cap), "slam_points_refine: ws_bytes %zu < %zu",
               ws_bytes, points_ws_bytes(n_frames, x_cap));
  PointsArgs a;
  a.rows = d_rows;
  a.count = d_count;
  a.poses = d_poses;
  a.P = d_P;
  a.X = d_X;
  a.n = d_n;
  a.tab = static_cast<int32_t*>(d_ws);
  a.status = d_status;
  a.nobs = d_nobs;
  a.cost = d_cost;
  a.info = d_info;
  a.var = d_var;
  a.mask = d_mask;
  a.nkilled = d_nkilled;
  a.n_frames = n_frames;
  a.rows_cap = rows_cap;
  a.x_cap = x_cap;
  a.loss = loss;
  a.n_rounds = n_rounds;
  a.iters = iters;
  a.min_obs = min_obs;
  a.kill = kill;
  a.loss_scale = loss_scale;
  a.gate = gate;
  a.min_depth = min_depth;
  a.max_var = max_var;
  hipStream_t s = slam::as_stream(stream);
  SLAM_HIP(hipMemsetAsync(d_ws, kNoRow & 0xff, points_ws_bytes(n_frames, x_cap), s));
  if (kill) SLAM_HIP(hipMemsetAsync(d_nkilled, 0, sizeof(int32_t), s));
  k_points_index<<<dim3(nblk(rows_cap, kWG), n_frames), kWG, 0, s>>>(a);
  SLAM_LAUNCHED("k_points_index");
  const unsigned nb = (unsigned)(((long long)x_cap + kLanes - 1) / kLanes);  // x_cap has no upper bound
  k_points_refine<<<nb, kLanes, 0, s>>>(a);
  SLAM_LAUNCHED("k_points_refine");
  return SLAM_OK;
}
