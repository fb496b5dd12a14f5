// Robust pose refinement from track rows (motion-only bundle adjustment): the
// step after guided matching.  slam_pose_refine in include/slam355.h states
// the definition; this file is its one kernel.
//
//   k_pose_refine   one 256-lane workgroup per frame -- a tracking batch is
//                   32-64 frames on 256 CUs and a frame is a dependent chain
//                   of n_rounds * iters LM iterations, so the latency of one
//                   frame is what there is to cut, not occupancy.  Lane t owns
//                   the observations t + 256 j; for j < kRc their Q = R^T (X -
//                   t), pixel and flags stay in registers for the whole call
//                   (the kRc idiom of k_pnp), the ones beyond recompute Q from
//                   the map each pass and keep their active flag in the output
//                   mask (read and written by the owning lane only).  The 28
//                   normal-equation sums go through wave_allsum32, the four
//                   wave partials to LDS rows of kRow doubles (the four writers
//                   on distinct banks), and every lane adds them in wave order:
//                   p and lambda stay replicated, every lane solves the same
//                   6x6 system and takes the same decision.  The trial cost
//                   and the inlier count take the same path.  Two workgroup
//                   barriers per LM iteration: the sums of the normal
//                   equations, of the trial and of the classification each
//                   have their own LDS buffer, so a buffer is rewritten only
//                   after a barrier that follows its last read.
#include "common.hpp"
#include "pose_math.hpp"
#include "robust_loss.hpp"

namespace {

constexpr int kWG = 256;
constexpr int kWaves = kWG / kWave;
constexpr int kRc = 4;    // observations per lane held in registers (count <= 1024 fully)
// LDS row of one wave's partial sums: 30 doubles = 60 dwords, so the rows of
// waves 0..3 start on banks 0, 60, 56, 52 (mod 64) and a ds_write_b128 of each
// of the four writers covers banks of its own.
constexpr int kRow = 30;
static_assert(kRow >= 28 && (2 * kRow) % 64 >= 4 && (2 * kRow) % 64 <= 60 && (2 * kRow) % 4 == 0,
              "wave rows on distinct banks");

struct RefineArgs {
  const double* rows;
  const int32_t* count;
  const double* X;
  const double* poses;
  const double* P;
  double* poses_out;
  uint8_t* mask;
  int32_t* ninl;
  int32_t* status;
  double* info;
  double* cost;
  int rows_cap, n_x, loss, n_rounds, iters, min_inliers;
  double loss_scale, gate, min_depth;
};

// X_cam = R Q + v in the operation order of pnp_residual
__device__ __forceinline__ void cam_point(const double p[6], const double R[9], const double* Q,
                                          double Xc[3], double RX[3]) {
  const double X0 = Q[0], X1 = Q[1], X2 = Q[2];
  RX[0] = R[0] * X0 + R[1] * X1 + R[2] * X2;
  RX[1] = R[3] * X0 + R[4] * X1 + R[5] * X2;
  RX[2] = R[6] * X0 + R[7] * X1 + R[8] * X2;
  Xc[0] = RX[0] + p[3];
  Xc[1] = RX[1] + p[4];
  Xc[2] = RX[2] + p[5];
}

// Residual of one observation (Q, xy) at p = (w, v) with R = Rod(w) under the
// 3x4 projection P, optionally its 2x6 Jacobian wrt (w, v); returns whether
// the observation is valid at p (depth above min_depth, h2 > 0).
template <bool JAC>
__device__ __forceinline__ bool pose_residual(const double p[6], const double R[9],
                                              const double* P, const double* Q, const double* xy,
                                              double min_depth, double r[2], double J[2][6]) {
  double Xc[3], RX[3], uv[2], a[2][3];
  cam_point(p, R, Q, Xc, RX);
  const double h2 = P[8] * Xc[0] + P[9] * Xc[1] + P[10] * Xc[2] + P[11];
  vo_project<JAC>(P, Xc, uv, a);
  r[0] = uv[0] - xy[0];
  r[1] = uv[1] - xy[1];
  if constexpr (JAC) {
    double D[3][3];
    drot_left(p, R, Q[0], Q[1], Q[2], RX[0], RX[1], RX[2], D);
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        J[c][k] = a[c][0] * D[0][k] + a[c][1] * D[1][k] + a[c][2] * D[2][k];
        J[c][3 + k] = a[c][k];
      }
  }
  return Xc[2] > min_depth && h2 > 0.0;
}

__global__ __launch_bounds__(kWG) void k_pose_refine(const RefineArgs a) {
  // [0] normal equations (and the final information), [1] trial, [2] classification
  __shared__ double red[3][kWaves * kRow];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & (kWave - 1), wid = t / kWave;
  const int n = min(max(a.count[b], 0), a.rows_cap);
  const double* rows = a.rows + (size_t)b * a.rows_cap * 4;
  uint8_t* mk = a.mask + (size_t)b * a.rows_cap;
  const double* T = a.poses + 16 * (size_t)b;
  double P[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) P[i] = a.P[i];
  const double gate2 = a.gate * a.gate;
  const int loss = a.loss;

  // observation i -> o = (Q, x, y); false when its landmark is not in the map
  auto load_obs = [&](int i, double o[5]) -> bool {
    const double* rw = rows + 4 * (size_t)i;
    const double l = rw[1];
    const bool ok = l >= 0.0 && l < (double)a.n_x;  // NaN: not ok
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    if (ok) {
      const double* x = a.X + 3 * (size_t)(int)l;
      x0 = x[0], x1 = x[1], x2 = x[2];
    }
    const double d0 = x0 - T[3], d1 = x1 - T[7], d2 = x2 - T[11];
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = T[k] * d0 + T[4 + k] * d1 + T[8 + k] * d2;
    o[3] = rw[2];
    o[4] = rw[3];
    return ok;
  };

  double rq[kRc][5];
  bool lok[kRc], act[kRc];
#pragma unroll
  for (int j = 0; j < kRc; ++j) {
    const int i = t + kWG * j;
    lok[j] = load_obs(min(i, max(n - 1, 0)), rq[j]) && i < n;
    act[j] = false;
  }
  // f(o, landmark ok, active&) for every observation of this lane; store: f
  // sets the flag (the mask holds nothing yet at the first classification).
  // The register slots are unrolled: with one wave per SIMD the independent
  // chains of a lane's observations are the only latency hiding there is (one
  // copy of f for all slots, the slot picked by selects, is half the code and
  // was not faster: profiles/pose_refine/).
  auto for_obs = [&](auto&& f, bool store) {
#pragma unroll
    for (int j = 0; j < kRc; ++j)
      if (kWG * j < n) {  // uniform
        f(rq[j], lok[j], act[j]);
        if (store && t + kWG * j < n) mk[t + kWG * j] = act[j] ? 1 : 0;
      }
    for (int i = t + kWG * kRc; i < n; i += kWG) {
      double o[5];
      const bool ok = load_obs(i, o);
      bool ac = !store && mk[i] != 0;
      f(o, ok, ac);
      if (store) mk[i] = ac ? 1 : 0;
    }
  };
  // workgroup sums of v[0..27], every lane ends with them (added in wave order)
  auto wg_sum28 = [&](double (&v)[32], int s) {
    wave_allsum32(v);
    double* rd = red[s];
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 28; ++k) rd[wid * kRow + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 28; ++k)
      v[k] = ((rd[k] + rd[kRow + k]) + rd[2 * kRow + k]) + rd[3 * kRow + k];
  };
  auto wg_sum2 = [&](double& x, double& y, int s) {
    x = wave_allsum(x);
    y = wave_allsum(y);
    double* rd = red[s];
    if (lane == 0) {
      rd[wid * kRow] = x;
      rd[wid * kRow + 1] = y;
    }
    __syncthreads();
    x = ((rd[0] + rd[kRow]) + rd[2 * kRow]) + rd[3 * kRow];
    y = ((rd[1] + rd[kRow + 1]) + rd[2 * kRow + 1]) + rd[3 * kRow + 1];
  };

  double p[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, R[9];
  rodrigues(p, R);

  // every observation: active iff valid at p and (gated) |r|^2 <= gate^2
  auto classify = [&](bool gated) -> int {
    double cnt = 0.0, none = 0.0;
    for_obs([&](const double* o, bool ok, bool& ac) {
      double r[2], J[2][6];
      const bool v = pose_residual<false>(p, R, P, o, o + 3, a.min_depth, r, J);
      ac = ok && v && (!gated || r[0] * r[0] + r[1] * r[1] <= gate2);
      cnt += ac ? 1.0 : 0.0;
    }, true);
    wg_sum2(cnt, none, 2);
    return (int)cnt;
  };
  // H (21), g (6) and the cost over the active set at p; relin: at the
  // increment 0 about the camera points of p (the information of the result)
  auto normal_sums = [&](double (&acc)[32], bool relin) {
#pragma unroll
    for (int i = 0; i < 32; ++i) acc[i] = 0.0;
    for_obs([&](const double* o, bool, bool& ac) {
      if (!ac) return;
      double pp[6], RR[9], QQ[3], Xc[3], RX[3];
      cam_point(p, R, o, Xc, RX);
#pragma unroll
      for (int i = 0; i < 6; ++i) pp[i] = relin ? 0.0 : p[i];
#pragma unroll
      for (int i = 0; i < 9; ++i) RR[i] = relin ? (i % 4 == 0 ? 1.0 : 0.0) : R[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) QQ[i] = relin ? Xc[i] : o[i];
      double r[2], J[2][6];
      pose_residual<true>(pp, RR, P, QQ, o + 3, a.min_depth, r, J);
      const double term = loss != 0 ? robust_weight<6>(r, J[0], J[1], loss, a.loss_scale)
                                    : r[0] * r[0] + r[1] * r[1];
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        int k = 0;
#pragma unroll
        for (int u = 0; u < 6; ++u) {
#pragma unroll
          for (int v = 0; v <= u; ++v) acc[k++] += J[c][u] * J[c][v];
          acc[21 + u] += J[c][u] * r[c];
        }
      }
      acc[27] += term;
    }, false);
    wg_sum28(acc, 0);
  };

  int status = 0;
  int na = classify(false);
  if (na < a.min_inliers) status = 1;
  for (int round = 0; round < a.n_rounds && status == 0; ++round) {
    double lam = 1e-3;
    for (int it = 0; it < a.iters; ++it) {
      double acc[32];
      normal_sums(acc, false);
      double H[21], g[6], d[6], pn[6], Rn[9];
#pragma unroll
      for (int i = 0; i < 21; ++i) H[i] = acc[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) g[i] = acc[21 + i];
      const double cost = acc[27];
      const bool ok = solve6(H, g, lam, d);
      for (int i = 0; i < 6; ++i) pn[i] = ok ? p[i] + d[i] : p[i];
      rodrigues(pn, Rn);
      double cn = 0.0, bad = 0.0;
      for_obs([&](const double* o, bool, bool& ac) {
        if (!ac) return;
        double r[2], J[2][6];
        if (!pose_residual<false>(pn, Rn, P, o, o + 3, a.min_depth, r, J)) bad += 1.0;
        cn += loss != 0 ? robust_weight<0>(r, nullptr, nullptr, loss, a.loss_scale)
                        : r[0] * r[0] + r[1] * r[1];
      }, false);
      wg_sum2(cn, bad, 1);
      if (ok && bad == 0.0 && cn < cost) {
        for (int i = 0; i < 6; ++i) p[i] = pn[i];
        for (int i = 0; i < 9; ++i) R[i] = Rn[i];
        lam = fmax(lam * 0.1, 1e-12);
      } else {
        lam = fmin(lam * 10.0, 1e12);
      }
    }
    na = classify(true);
    if (na < a.min_inliers) status = 2;
  }

  double* To = a.poses_out + 16 * (size_t)b;
  double* info = a.info + 36 * (size_t)b;
  if (status != 0) {  // the input pose bit for bit, zeros, -1
    if (t < 16) To[t] = T[t];
    if (t < 36) info[t] = 0.0;
    if (t == 0) {
      a.ninl[b] = -1;
      a.status[b] = status;
      a.cost[b] = 0.0;
    }
    return;
  }
  double acc[32];
  normal_sums(acc, true);
  if (t == 0) {
    // R' = R Rod(w)^T, t' = t - R' v
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double Ri[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        Ri[j] = T[4 * i] * R[3 * j] + T[4 * i + 1] * R[3 * j + 1] + T[4 * i + 2] * R[3 * j + 2];
        To[4 * i + j] = Ri[j];
      }
      To[4 * i + 3] = T[4 * i + 3] - (Ri[0] * p[3] + Ri[1] * p[4] + Ri[2] * p[5]);
    }
    To[12] = 0.0; To[13] = 0.0; To[14] = 0.0; To[15] = 1.0;
    a.ninl[b] = na;
    a.status[b] = 0;
    a.cost[b] = acc[27];
  }
  if (t == kWave) {  // a lane of the second wave: the 6x6 information, both triangles
    int k = 0;
#pragma unroll
    for (int u = 0; u < 6; ++u)
#pragma unroll
      for (int v = 0; v <= u; ++v) {
        info[6 * u + v] = acc[k];
        info[6 * v + u] = acc[k];
        ++k;
      }
  }
}

}  // namespace

extern "C" int slam_pose_refine(const double* d_rows, const int32_t* d_count, int rows_cap,
                                int batch, const double* d_X, int n_x, const double* d_poses,
                                const double* d_P, int loss, double loss_scale, double gate,
                                double min_depth, int n_rounds, int iters, int min_inliers,
                                double* d_poses_out, uint8_t* d_mask, int32_t* d_ninl,
                                int32_t* d_status, double* d_info, double* d_cost, void* stream) {
  SLAM_REQUIRE(d_rows && d_count && d_X && d_poses && d_P && d_poses_out && d_mask && d_ninl &&
                   d_status && d_info && d_cost,
               "slam_pose_refine: null pointer");
  SLAM_REQUIRE(batch >= 1 && batch <= 65535, "slam_pose_refine: batch %d not in 1..65535", batch);
  SLAM_REQUIRE(rows_cap >= 1 && rows_cap <= 65535, "slam_pose_refine: rows_cap %d not in 1..65535",
               rows_cap);
  SLAM_REQUIRE(n_x >= 0, "slam_pose_refine: n_x %d < 0", n_x);
  SLAM_REQUIRE(n_rounds >= 1 && n_rounds <= 8, "slam_pose_refine: n_rounds %d not in 1..8",
               n_rounds);
  SLAM_REQUIRE(iters >= 1 && iters <= 50, "slam_pose_refine: iters %d not in 1..50", iters);
  SLAM_REQUIRE(min_inliers >= 3, "slam_pose_refine: min_inliers %d < 3", min_inliers);
  SLAM_REQUIRE(loss >= 0 && loss <= 3, "slam_pose_refine: loss %d not in 0..3", loss);
  SLAM_REQUIRE(loss == 0 || loss_scale > 0.0, "slam_pose_refine: loss_scale must be > 0");
  SLAM_REQUIRE(gate > 0.0, "slam_pose_refine: gate must be > 0");  // NaN refused too
  SLAM_REQUIRE(min_depth == min_depth, "slam_pose_refine: min_depth is NaN");
  RefineArgs a;
  a.rows = d_rows;
  a.count = d_count;
  a.X = d_X;
  a.poses = d_poses;
  a.P = d_P;
  a.poses_out = d_poses_out;
  a.mask = d_mask;
  a.ninl = d_ninl;
  a.status = d_status;
  a.info = d_info;
  a.cost = d_cost;
  a.rows_cap = rows_cap;
  a.n_x = n_x;
  a.loss = loss;
  a.n_rounds = n_rounds;
  a.iters = iters;
  a.min_inliers = min_inliers;
  a.loss_scale = loss_scale;
  a.gate = gate;
  a.min_depth = min_depth;
  k_pose_refine<<<batch, kWG, 0, slam::as_stream(stream)>>>(a);
  SLAM_LAUNCHED("k_pose_refine");
  return SLAM_OK;
}
