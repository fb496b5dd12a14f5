// Covariance of a bundle-adjustment estimate: camera blocks, landmark blocks and
// landmark-camera blocks of the inverse of the normal equations at lambda = 0.
// The build is ba.hip's (slam::make_launch / slam::launch_build, ba_common.hpp),
// the per-observation Jacobian ba_project.hpp's, the tile steps tile_f64.hpp's.
#include "ba_common.hpp"
#include "ba_layout.hpp"
#include "ba_project.hpp"
#include "tile_f64.hpp"

using slam::Launch;

// ---------------------------------------------------------------- camera covariance
// Marginal covariance of the camera parameters: 9x9 blocks of S0^-1, S0 the
// reduced camera system at lambda = 0.  The build runs unchanged
// between two one-lane kernels that park lambda; S0 is gathered into lower
// 64x64 tiles of a dense matrix in natural camera order (held and padding rows:
// unit diagonal, no coupling), factored by a blocked right-looking Cholesky over
// tile columns (k_cov_panel / k_cov_update, the tile factor of the tiled
// solve), L^-1 formed by tile rows (k_cov_minv), and the requested tiles of
// L^-T L^-1 (k_cov_sigma) picked into the output blocks (k_cov_pick).  Not a
// per-iteration path: one workgroup per tile, O(T) launches, nothing resident.
namespace {

struct CovLayout {  // doubles inside the workspace; T = ceil(9C / 64)
  int T, N;
  long long a, m, diag, need, hdr, total;
  __host__ __device__ explicit CovLayout(int n_cams) {
    T = (9 * n_cams + kTB - 1) / kTB;
    N = T * kTB;
    a = 0;                              // S0 -> L (lower tiles), then the tiles of Sigma
    m = a + (long long)N * N;           // L^-1 (lower tiles; the diagonal tiles hold L_kk^-1)
    diag = m + (long long)N * N;        // diagonal of S0 (1 on held and padding rows)
    need = diag + N;                    // ints [T][T]: lower tile (I, J) holds a requested entry
    hdr = need + ((long long)T * T + 1) / 2;  // [0] the parked lambda, [1] (int) status
    total = hdr + 8;
  }
};

__device__ __forceinline__ bool cov_free(const slam_ba_problem& p, int r) {
  if (r >= 9 * p.n_cams) return false;
  return p.cam_fixed == nullptr || ((p.cam_fixed[r / 9] >> (r % 9)) & 1u) == 0;
}
__device__ __forceinline__ bool cov_failed(const double* ws, const CovLayout& L) {
  return *reinterpret_cast<const volatile int*>(ws + L.hdr + 1) != 0;
}

// restore == 0: lambda parked in the workspace and set to 0, status cleared;
// restore == 1: lambda back.  No other state slot is touched.
__global__ void k_cov_lambda(slam_ba_problem p, double* ws, int restore) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const CovLayout L(p.n_cams);
  if (restore) {
    p.state[SLAM_BA_ST_LAMBDA] = ws[L.hdr];
  } else {
    ws[L.hdr] = p.state[SLAM_BA_ST_LAMBDA];
    p.state[SLAM_BA_ST_LAMBDA] = 0.0;
    *reinterpret_cast<int*>(ws + L.hdr + 1) = 0;
  }
}

// One workgroup per lower tile: S0 from the dense sys (zeros for a packed one,
// k_cov_scatter follows), identity on held and padding rows; the diagonal of S0.
__global__ __launch_bounds__(kTlWG) void k_cov_load(slam_ba_problem p, double* ws) {
  const CovLayout L(p.n_cams);
  const int n = 9 * p.n_cams;
  const int2 IJ = lower_tile_of(blockIdx.x);
  const bool dense = !sys_packed(p.n_cams);
  double* A = ws + L.a;
  for (int e = threadIdx.x; e < kTB * kTB; e += kTlWG) {
    const int i = IJ.x * kTB + (e >> 6), j = IJ.y * kTB + (e & 63);
    double v = i == j ? 1.0 : 0.0;
    if (cov_free(p, i) && cov_free(p, j)) v = dense ? p.sys[(size_t)i * n + j] : 0.0;
    A[(size_t)i * L.N + j] = v;
  }
  if (IJ.x == IJ.y && threadIdx.x < kTB) {
    const int i = IJ.x * kTB + threadIdx.x;
    if (!cov_free(p, i)) ws[L.diag + i] = 1.0;
    else if (dense) ws[L.diag + i] = p.sys[(size_t)i * n + i];
  }
  if (threadIdx.x == 0) reinterpret_cast<int*>(ws + L.need)[IJ.x * L.T + IJ.y] = 0;
}

// One workgroup per packed block: its free entries into the lower tiles (both
// triangles inside a diagonal tile), the diagonal of S0.
__global__ __launch_bounds__(128) void k_cov_scatter(slam_ba_problem p, double* ws) {
  const CovLayout L(p.n_cams);
  const int blk = blockIdx.x, t = threadIdx.x;
  if (t >= 81) return;
  const int c1 = p.blocks[2 * blk], c2 = p.blocks[2 * blk + 1];
  const int r = 9 * c1 + t / 9, c = 9 * c2 + t % 9;
  if (!cov_free(p, r) || !cov_free(p, c)) return;
  const double v = p.sys[(size_t)blk * 81 + t];
  double* A = ws + L.a;
  const int tr = r / kTB, tc = c / kTB;
  if (tr >= tc) A[(size_t)r * L.N + c] = v;
  if (c1 != c2 && tc >= tr) A[(size_t)c * L.N + r] = v;
  if (r == c) ws[L.diag + r] = v;
}

// The lower tiles that hold an entry of a requested block (a block may straddle tiles).
__global__ __launch_bounds__(kBS) void k_cov_mark(slam_ba_problem p, const int32_t* __restrict__ pairs,
                                                  int n_pairs, double* ws) {
  const CovLayout L(p.n_cams);
  const int q = blockIdx.x * kBS + threadIdx.x;
  if (q >= n_pairs) return;
  const int a = pairs[2 * q], b = pairs[2 * q + 1];
  if ((unsigned)a >= (unsigned)p.n_cams || (unsigned)b >= (unsigned)p.n_cams) return;
  int* need = reinterpret_cast<int*>(ws + L.need);
  for (int ta = 9 * a / kTB; ta <= (9 * a + 8) / kTB; ++ta)
    for (int tb = 9 * b / kTB; tb <= (9 * b + 8) / kTB; ++tb) need[max(ta, tb) * L.T + min(ta, tb)] = 1;
}

// Tile column k, one workgroup per tile (I, k), I = k + blockIdx.x: every one
// factors A_kk (tile_chol_inv_blk: L_kk^-1); the diagonal one stores L_kk^-1 as
// the diagonal tile of L^-1 and runs the relative-pivot test, the others form
// L_Ik = A_Ik L_kk^-T in place.
__global__ __launch_bounds__(kTlWG) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_cov_panel(slam_ba_problem p, double* ws, int k, double rank_tol) {
  const CovLayout L(p.n_cams);
  const int rows = min(kTB, 9 * p.n_cams - k * kTB);
  int* fail = reinterpret_cast<int*>(ws + L.hdr + 1);
  tile_panel(DenseTiles(ws + L.a, L.N), k, k + (int)blockIdx.x, (rows + 15) >> 4, fail,
             [&](const double (&x)[kTB], bool ok, int lane, double*) {
               double* Mkk = ws + L.m + (size_t)k * kTB * L.N + k * kTB;
#pragma unroll
               for (int m = 0; m < kTB; ++m) Mkk[(size_t)m * L.N + lane] = x[m];
               // pivot d = L_cc^2 = 1 / (L_kk^-1)_cc^2 against rank_tol * S0_cc
               double xd = 0.0;
#pragma unroll
               for (int m = 0; m < kTB; ++m) xd = m == lane ? x[m] : xd;
               const double piv = 1.0 / (xd * xd);
               const bool bad = !ok || !(xd > 0.0 && xd < INFINITY) || !(piv < INFINITY) ||
                                piv <= rank_tol * ws[L.diag + k * kTB + lane];
               if (__any(bad) && lane == 0) *fail = 1;
             });
}

// Trailing update of column k, one workgroup per tile (I, J), I >= J > k:
// A_IJ -= L_Ik L_Jk^T.
__global__ __launch_bounds__(kTlWG) void k_cov_update(slam_ba_problem p, double* ws, int k) {
  const CovLayout L(p.n_cams);
  if (cov_failed(ws, L)) return;
  const int2 IJ = lower_tile_of(blockIdx.x);
  tile_update<false>(DenseTiles(ws + L.a, L.N), k + 1 + IJ.x, k + 1 + IJ.y, k, nullptr, nullptr);
}

// Tile row i of M = L^-1, one workgroup per tile (i, j), j < i:
// M_ij = -L_ii^-1 sum_{k=j}^{i-1} L_ik M_kj  (rows < i of M are complete).
__global__ __launch_bounds__(kTlWG) void k_cov_minv(slam_ba_problem p, double* ws, int i) {
  const CovLayout L(p.n_cams);
  if (cov_failed(ws, L)) return;
  const int j = blockIdx.x;
  __shared__ double Xf[kTB * kTB], Yf[kTB * kTB];
  const double* A = ws + L.a;
  double* M = ws + L.m;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  d4 acc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
  for (int k = j; k < i; ++k) {
    tile_to_frag(A + (size_t)i * kTB * L.N + k * kTB, L.N, Xf);
    tile_to_frag_t(M + (size_t)k * kTB * L.N + j * kTB, L.N, Yf);
    __syncthreads();
    tile_gemm_acc(Xf, Yf, acc);
    __syncthreads();  // Xf / Yf reloaded next k
  }
  tile_to_frag(M + (size_t)i * kTB * L.N + i * kTB, L.N, Xf);
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      Yf[frag_idx(s * 16 + (lane & 15), w * 16 + (lane >> 4) + 4 * r)] = acc[s][r];  // the sum, transposed image
  __syncthreads();
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
  tile_gemm_acc(Xf, Yf, acc, true);
  tile_store(M + (size_t)i * kTB * L.N + j * kTB, L.N, acc);
}

// Sigma_IJ = sum_{k >= I} M_kI^T M_kJ for the marked lower tiles (I >= J), into
// the tiles of the factor (dead by now).
__global__ __launch_bounds__(kTlWG) void k_cov_sigma(slam_ba_problem p, double* ws) {
  const CovLayout L(p.n_cams);
  if (cov_failed(ws, L)) return;
  const int2 IJ = lower_tile_of(blockIdx.x);
  const int I = IJ.x, J = IJ.y;
  if (reinterpret_cast<const int*>(ws + L.need)[I * L.T + J] == 0) return;
  __shared__ double Xf[kTB * kTB], Yf[kTB * kTB];
  const double* M = ws + L.m;
  d4 acc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
  for (int k = I; k < L.T; ++k) {
    tile_to_frag_t(M + (size_t)k * kTB * L.N + I * kTB, L.N, Xf);
    if (I != J) tile_to_frag_t(M + (size_t)k * kTB * L.N + J * kTB, L.N, Yf);
    __syncthreads();
    tile_gemm_acc(Xf, I == J ? Xf : Yf, acc);
    __syncthreads();
  }
  tile_store(ws + L.a + (size_t)I * kTB * L.N + J * kTB, L.N, acc);
}

// One workgroup per requested block: entry (i, j) from the lower triangle of
// Sigma (so a marginal block is exactly symmetric and block (a, b) is block
// (b, a) transposed bit for bit), +0.0 on held rows and columns, NaN when the
// system was not positive definite; the status.
__global__ __launch_bounds__(128) void k_cov_pick(slam_ba_problem p, const int32_t* __restrict__ pairs,
                                                  const double* __restrict__ ws, double* __restrict__ cov,
                                                  int32_t* __restrict__ status) {
  const CovLayout L(p.n_cams);
  const bool failed = cov_failed(ws, L);
  const int q = blockIdx.x, t = threadIdx.x;
  if (q == 0 && t == 0) status[0] = failed ? 1 : 0;
  if (t >= 81) return;
  const int a = pairs[2 * q], b = pairs[2 * q + 1];
  double v = __builtin_nan("");
  if (!failed && (unsigned)a < (unsigned)p.n_cams && (unsigned)b < (unsigned)p.n_cams) {
    const int i = 9 * a + t / 9, j = 9 * b + t % 9;
    v = 0.0;
    if (cov_free(p, i) && cov_free(p, j)) v = ws[L.a + (size_t)max(i, j) * L.N + min(i, j)];
  }
  cov[(size_t)q * 81 + t] = v;
}

// ---------------------------------------------------------------- landmark covariance
// Point blocks Sigma_pp and point-camera blocks Sigma_pc of the same inverse
// (DESIGN.md 4c), from Sigma_cc as k_cov_sigma left it: per observation o of a
// point, J~ = (Jc | Jp) as k_linearize forms it, and
//   Sigma_pp = V^-1 + V^-1 (sum_{o,o'} Jp_o^T (Jc_o Sigma_{c(o)c(o')} Jc_o'^T) Jp_o') V^-1,
//   Sigma_pc = -V^-1 sum_o Jp_o^T (Jc_o Sigma_{c(o),c}),      V = sum_o Jp_o^T Jp_o
// (W_o^T Sigma W_o' with W = Jc^T Jp, the 2 x 2 middle factor formed first:
// 24 staged doubles per observation instead of 33, 230 multiplies per pair
// instead of 324).  One wave per requested entry, kCovPW entries per
// workgroup; the waves never meet (no __syncthreads), sums are fixed shuffle
// trees, so an entry's bits do not depend on the request around it.
constexpr int kCovPW = 4;   // waves per workgroup
constexpr int kCovCh = 8;   // observations per chunk: a step covers the 8 x 8 ordered pairs of two chunks
constexpr int kCovJS = 25;  // LDS stride of a staged 2 x 12 Jacobian (odd: rows spread over the banks)

__device__ __forceinline__ double cov_sig(const double* __restrict__ ws, const CovLayout& L, int i, int j) {
  return ws[L.a + (size_t)max(i, j) * L.N + min(i, j)];
}

// J~ of observation o: the steps of k_linearize in its order
__device__ __forceinline__ void cov_obs_jac(const slam_ba_problem& p, int cur, int o, double J[2][12]) {
  double r[2];
  const int c = p.obs_cam[o];
  reproject_pre<true>(p.camrec[cur] + kCamRec * c, p.pts[cur] + 3 * p.obs_pt[o], p.obs_q + 2 * o, r, J);
  clamp_rows<true>(r, J);
  if (p.cam_fixed != nullptr) hold_cols(J, p.cam_fixed[c]);
  if (p.loss != 0) robust_weight<12>(r, J[0], J[1], p.loss, p.loss_scale);
}

// the tree of block_sum over one wave; the sum on every lane
__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return __shfl(v, 0, 64);
}

__device__ __forceinline__ void cov_mark_block(int* need, int T, int a, int b) {
  for (int ta = 9 * a / kTB; ta <= (9 * a + 8) / kTB; ++ta)
    for (int tb = 9 * b / kTB; tb <= (9 * b + 8) / kTB; ++tb) need[max(ta, tb) * T + min(ta, tb)] = 1;
}

// The lower tiles the point and cross requests read: blocks (c(o), c(o')) of a
// requested point, (c(o), c) of a requested (point, camera).  One lane per entry.
__global__ __launch_bounds__(kBS) void k_cov_mark_pts(slam_ba_problem p, const int32_t* __restrict__ points,
                                                      int n_points, const int32_t* __restrict__ cross,
                                                      int n_cross, double* ws) {
  const CovLayout L(p.n_cams);
  const int q = blockIdx.x * kBS + threadIdx.x;
  if (q >= n_points + n_cross) return;
  int* need = reinterpret_cast<int*>(ws + L.need);
  const bool is_pt = q < n_points;
  const int pt = is_pt ? (points ? points[q] : q) : cross[2 * (q - n_points)];
  const int c = is_pt ? 0 : cross[2 * (q - n_points) + 1];
  if ((unsigned)pt >= (unsigned)p.n_pts || (unsigned)c >= (unsigned)p.n_cams) return;
  const int o0 = p.pt_ptr[pt], o1 = p.pt_ptr[pt + 1];
  for (int o = o0; o < o1; ++o) {
    const int a = p.obs_cam[o];
    if (!is_pt) {
      cov_mark_block(need, L.T, a, c);
      continue;
    }
    for (int o2 = o0; o2 <= o; ++o2) cov_mark_block(need, L.T, a, p.obs_cam[o2]);  // (a, b) and (b, a): one lower tile
  }
}

// Both status words of slam_ba_covariance_points, before the kernels that count.
__global__ void k_cov_status(slam_ba_problem p, const double* __restrict__ ws, int32_t* __restrict__ status) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  status[0] = cov_failed(ws, CovLayout(p.n_cams)) ? 1 : 0;
  status[1] = 0;
}

// V^-1 of point pt by a whole wave, the same on every lane: lanes over the
// observations, the six sums by wave_sum, the pivots of the unpivoted 3x3
// Cholesky (as squares: d_k of L D L^T) against rank_tol V_kk, the inverse by
// cofactors.  false: the point is undetermined.
__device__ __forceinline__ bool cov_point_vinv(const slam_ba_problem& p, int cur, int pt, double rank_tol,
                                               double iv[6]) {
  const int lane = threadIdx.x & 63;
  const int o0 = p.pt_ptr[pt], o1 = p.pt_ptr[pt + 1];
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int ob = o0; ob < o1; ob += 64) {
    const int o = ob + lane;
    if (o < o1) {
      double J[2][12];
      cov_obs_jac(p, cur, o, J);
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        v[0] += J[a][9] * J[a][9];
        v[1] += J[a][9] * J[a][10];
        v[2] += J[a][9] * J[a][11];
        v[3] += J[a][10] * J[a][10];
        v[4] += J[a][10] * J[a][11];
        v[5] += J[a][11] * J[a][11];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) v[k] = wave_sum(v[k]);
  const double a00 = v[0], a01 = v[1], a02 = v[2], a11 = v[3], a12 = v[4], a22 = v[5];
  const double d0 = a00;
  const double l10 = a01 / d0, l20 = a02 / d0;
  const double d1 = a11 - l10 * a01;
  const double u21 = a12 - l20 * a01;
  const double d2 = a22 - l20 * a02 - (u21 / d1) * u21;
  const double c00 = a11 * a22 - a12 * a12;
  const double c01 = a02 * a12 - a01 * a22;
  const double c02 = a01 * a12 - a02 * a11;
  const double c11 = a00 * a22 - a02 * a02;
  const double c12 = a01 * a02 - a00 * a12;
  const double c22 = a00 * a11 - a01 * a01;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  const bool ok = d0 > rank_tol * a00 && d0 < INFINITY && d1 > rank_tol * a11 && d1 < INFINITY &&
                  d2 > rank_tol * a22 && d2 < INFINITY && det > 0.0 && det < INFINITY;  // (a NaN fails every test)
  const double id = 1.0 / det;
  iv[0] = c00 * id; iv[1] = c01 * id; iv[2] = c02 * id;
  iv[3] = c11 * id; iv[4] = c12 * id; iv[5] = c22 * id;
  return ok;
}

// Sigma_pp of the requested points, [n_points][3][3].  A wave walks the pairs of
// 8-observation chunks (A, B) of its point: lanes 0..15 stage the J~ of the two
// chunks in LDS (recomputed per step: nothing of the point is kept beyond 16
// rows, so a deep point needs no more LDS than a shallow one), lane (a, b)
// adds observation pair (8A + a, 8B + b) to its six entries.
__global__ __launch_bounds__(64 * kCovPW) void k_cov_points(slam_ba_problem p, const int32_t* __restrict__ points,
                                                            int n_points, double rank_tol,
                                                            const double* __restrict__ ws,
                                                            double* __restrict__ cov_pp,
                                                            int32_t* __restrict__ status) {
  __shared__ double Js[kCovPW][2 * kCovCh][kCovJS];
  __shared__ int Cs[kCovPW][2 * kCovCh];
  const CovLayout L(p.n_cams);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = blockIdx.x * kCovPW + w;
  if (q >= n_points) return;
  const int pt = points ? points[q] : q;
  double* out = cov_pp + (size_t)q * 9;
  if (cov_failed(ws, L) || (unsigned)pt >= (unsigned)p.n_pts) {
    if (lane < 9) out[lane] = __builtin_nan("");
    return;
  }
  const int cur = cur_of(p.state);
  double iv[6];
  if (!cov_point_vinv(p, cur, pt, rank_tol, iv)) {
    if (lane < 9) out[lane] = __builtin_nan("");
    if (lane == 0) atomicAdd(status + 1, 1);
    return;
  }
  const int o0 = p.pt_ptr[pt], n = p.pt_ptr[pt + 1] - o0;
  const int nch = (n + kCovCh - 1) / kCovCh;
  const int a = lane >> 3, b = lane & 7;
  double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int A = 0; A < nch; ++A)
    for (int B = 0; B < nch; ++B) {
      if (lane < 2 * kCovCh) {
        const int k = (lane < kCovCh ? A : B) * kCovCh + (lane & (kCovCh - 1));
        if (k < n) {
          double J[2][12];
          cov_obs_jac(p, cur, o0 + k, J);
#pragma unroll
          for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int i = 0; i < 12; ++i) Js[w][lane][12 * r + i] = J[r][i];
          Cs[w][lane] = p.obs_cam[o0 + k];
        }
      }
      wave_lds_fence();
      if (A * kCovCh + a < n && B * kCovCh + b < n) {
        const double* Ja = Js[w][a];
        const double* Jb = Js[w][kCovCh + b];
        const int ia = 9 * Cs[w][a], ib = 9 * Cs[w][kCovCh + b];
        double g00 = 0.0, g01 = 0.0, g10 = 0.0, g11 = 0.0;  // Jc_a Sigma_{c(a) c(b)} Jc_b^T
        for (int s = 0; s < 9; ++s) {
          double t0 = 0.0, t1 = 0.0;
#pragma unroll
          for (int r = 0; r < 9; ++r) {
            const double sg = cov_sig(ws, L, ia + r, ib + s);
            t0 += Ja[r] * sg;
            t1 += Ja[12 + r] * sg;
          }
          g00 += t0 * Jb[s];
          g01 += t0 * Jb[12 + s];
          g10 += t1 * Jb[s];
          g11 += t1 * Jb[12 + s];
        }
        int e = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const double h0 = Ja[9 + i] * g00 + Ja[21 + i] * g10, h1 = Ja[9 + i] * g01 + Ja[21 + i] * g11;
#pragma unroll
          for (int j = i; j < 3; ++j) m[e++] += h0 * Jb[9 + j] + h1 * Jb[21 + j];
        }
      }
      wave_lds_fence();  // the rows are staged again in the next step
    }
#pragma unroll
  for (int k = 0; k < 6; ++k) m[k] = wave_sum(m[k]);
  if (lane != 0) return;
  // V^-1 + V^-1 (M V^-1): six entries, mirrored
  const double M[3][3] = {{m[0], m[1], m[2]}, {m[1], m[3], m[4]}, {m[2], m[4], m[5]}};
  const double IV[3][3] = {{iv[0], iv[1], iv[2]}, {iv[1], iv[3], iv[4]}, {iv[2], iv[4], iv[5]}};
  double X[3][3], S[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) X[i][j] = M[i][0] * IV[0][j] + M[i][1] * IV[1][j] + M[i][2] * IV[2][j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j)
      S[i][j] = S[j][i] = IV[i][j] + (IV[i][0] * X[0][j] + IV[i][1] * X[1][j] + IV[i][2] * X[2][j]);
#pragma unroll
  for (int i = 0; i < 9; ++i) out[i] = S[i / 3][i % 3];
}

// Sigma_pc of the requested (point, camera) entries, [n_cross][3][9]: lanes over
// the point's observations, 27 sums by wave_sum, then -V^-1 . ; +0.0 in the
// columns of held parameters of the camera.
__global__ __launch_bounds__(64 * kCovPW) void k_cov_cross(slam_ba_problem p, const int32_t* __restrict__ cross,
                                                           int n_cross, double rank_tol,
                                                           const double* __restrict__ ws,
                                                           double* __restrict__ cov_pc,
                                                           int32_t* __restrict__ status) {
  const CovLayout L(p.n_cams);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = blockIdx.x * kCovPW + w;
  if (q >= n_cross) return;
  const int pt = cross[2 * q], c = cross[2 * q + 1];
  double* out = cov_pc + (size_t)q * 27;
  if (cov_failed(ws, L) || (unsigned)pt >= (unsigned)p.n_pts || (unsigned)c >= (unsigned)p.n_cams) {
    if (lane < 27) out[lane] = __builtin_nan("");
    return;
  }
  const int cur = cur_of(p.state);
  double iv[6];
  if (!cov_point_vinv(p, cur, pt, rank_tol, iv)) {
    if (lane < 27) out[lane] = __builtin_nan("");
    if (lane == 0) atomicAdd(status + 1, 1);
    return;
  }
  const int o0 = p.pt_ptr[pt], o1 = p.pt_ptr[pt + 1];
  double acc[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) acc[k] = 0.0;
  for (int ob = o0; ob < o1; ob += 64) {
    const int o = ob + lane;
    if (o < o1) {
      double J[2][12];
      cov_obs_jac(p, cur, o, J);
      const int ia = 9 * p.obs_cam[o];
#pragma unroll
      for (int s = 0; s < 9; ++s) {
        double t0 = 0.0, t1 = 0.0;  // (Jc_o Sigma_{c(o), c})[:, s]
#pragma unroll
        for (int r = 0; r < 9; ++r) {
          const double sg = cov_sig(ws, L, ia + r, 9 * c + s);
          t0 += J[0][r] * sg;
          t1 += J[1][r] * sg;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) acc[9 * i + s] += J[0][9 + i] * t0 + J[1][9 + i] * t1;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 27; ++k) acc[k] = wave_sum(acc[k]);
  if (lane != 0) return;
  const unsigned fx = p.cam_fixed != nullptr ? p.cam_fixed[c] : 0u;
  const double IV[3][3] = {{iv[0], iv[1], iv[2]}, {iv[1], iv[3], iv[4]}, {iv[2], iv[4], iv[5]}};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int s = 0; s < 9; ++s) {
      const double v = 0.0 - (IV[i][0] * acc[s] + IV[i][1] * acc[9 + s] + IV[i][2] * acc[18 + s]);  // (never -0.0)
      out[9 * i + s] = ((fx >> s) & 1u) ? 0.0 : v;
    }
}

}  // namespace

extern "C" long long slam_ba_cov_workspace_len(int n_cams) {
  if (n_cams <= 0) return 0;
  return CovLayout(n_cams).total;
}

namespace {

struct CovRequest {
  const int32_t* pairs;   int n_pairs;  double* cov;      // camera blocks (k_cov_mark, k_cov_pick)
  const int32_t* points;  int n_points; double* cov_pp;   // point blocks (null list: every point in order)
  const int32_t* cross;   int n_cross;  double* cov_pc;   // (point, camera) blocks
  bool two_words;                                         // d_status [2] (slam_ba_covariance_points)
};

// The launches of both covariance entry points: one build at lambda = 0, one
// factorisation, Sigma on the marked tiles, then the requested blocks.
int cov_launch(const Launch& La, const CovRequest& rq, double rank_tol, double* d_ws, int32_t* d_status,
               hipStream_t s) {
  const slam_ba_problem& p = La.b.p[0];
  const int T = CovLayout(p.n_cams).T;
  k_cov_lambda<<<1, 64, 0, s>>>(p, d_ws, 0);
  SLAM_LAUNCHED("k_cov_lambda");
  const int rc = launch_build(La, s);
  k_cov_lambda<<<1, 64, 0, s>>>(p, d_ws, 1);  // also after a failed launch: lambda goes back
  SLAM_LAUNCHED("k_cov_lambda");
  if (rc) return rc;
  k_cov_load<<<T * (T + 1) / 2, kTlWG, 0, s>>>(p, d_ws);
  SLAM_LAUNCHED("k_cov_load");
  if (sys_packed(p.n_cams)) {
    k_cov_scatter<<<p.n_blocks, 128, 0, s>>>(p, d_ws);
    SLAM_LAUNCHED("k_cov_scatter");
  }
  if (rq.n_pairs > 0) {
    k_cov_mark<<<nblk(rq.n_pairs, kBS), kBS, 0, s>>>(p, rq.pairs, rq.n_pairs, d_ws);
    SLAM_LAUNCHED("k_cov_mark");
  }
  if (rq.n_points + rq.n_cross > 0) {
    k_cov_mark_pts<<<nblk(rq.n_points + rq.n_cross, kBS), kBS, 0, s>>>(p, rq.points, rq.n_points, rq.cross,
                                                                      rq.n_cross, d_ws);
    SLAM_LAUNCHED("k_cov_mark_pts");
  }
  for (int k = 0; k < T; ++k) {
    k_cov_panel<<<T - k, kTlWG, 0, s>>>(p, d_ws, k, rank_tol);
    SLAM_LAUNCHED("k_cov_panel");
    const int m = T - k - 1;
    if (m > 0) {
      k_cov_update<<<m * (m + 1) / 2, kTlWG, 0, s>>>(p, d_ws, k);
      SLAM_LAUNCHED("k_cov_update");
    }
  }
  for (int i = 1; i < T; ++i) {
    k_cov_minv<<<i, kTlWG, 0, s>>>(p, d_ws, i);
    SLAM_LAUNCHED("k_cov_minv");
  }
  k_cov_sigma<<<T * (T + 1) / 2, kTlWG, 0, s>>>(p, d_ws);
  SLAM_LAUNCHED("k_cov_sigma");
  if (rq.two_words) {
    k_cov_status<<<1, 64, 0, s>>>(p, d_ws, d_status);
    SLAM_LAUNCHED("k_cov_status");
  }
  if (rq.n_pairs > 0) {
    k_cov_pick<<<rq.n_pairs, 128, 0, s>>>(p, rq.pairs, d_ws, rq.cov, d_status);
    SLAM_LAUNCHED("k_cov_pick");
  }
  if (rq.n_points > 0) {
    k_cov_points<<<nblk(rq.n_points, kCovPW), 64 * kCovPW, 0, s>>>(p, rq.points, rq.n_points, rank_tol, d_ws,
                                                                  rq.cov_pp, d_status);
    SLAM_LAUNCHED("k_cov_points");
  }
  if (rq.n_cross > 0) {
    k_cov_cross<<<nblk(rq.n_cross, kCovPW), 64 * kCovPW, 0, s>>>(p, rq.cross, rq.n_cross, rank_tol, d_ws,
                                                                rq.cov_pc, d_status);
    SLAM_LAUNCHED("k_cov_cross");
  }
  return SLAM_OK;
}

}  // namespace

extern "C" int slam_ba_covariance(const slam_ba_problem* prob, const int32_t* d_pairs, int n_pairs,
                                  double rank_tol, double* d_cov, double* d_ws, long long ws_len,
                                  int32_t* d_status, void* stream) {
  Launch La;
  if (int rc = make_launch(prob, 1, &La)) return rc;
  SLAM_REQUIRE(n_pairs >= 1, "slam_ba_covariance: n_pairs %d < 1", n_pairs);
  SLAM_REQUIRE(std::isfinite(rank_tol) && rank_tol >= 0.0 && rank_tol < 1.0,
               "slam_ba_covariance: rank_tol %g must be finite and in [0, 1)", rank_tol);
  SLAM_REQUIRE(d_pairs && d_cov && d_status, "slam_ba_covariance: null pointer");
  const CovLayout L(prob->n_cams);
  SLAM_REQUIRE(d_ws != nullptr && ws_len >= L.total,
               "slam_ba_covariance: workspace of %lld doubles, slam_ba_cov_workspace_len gives %lld",
               d_ws ? ws_len : 0ll, L.total);
  const CovRequest rq{d_pairs, n_pairs, d_cov, nullptr, 0, nullptr, nullptr, 0, nullptr, false};
  return cov_launch(La, rq, rank_tol, d_ws, d_status, slam::as_stream(stream));
}

extern "C" int slam_ba_covariance_points(const slam_ba_problem* prob, const int32_t* d_pairs, int n_pairs,
                                         double* d_cov, const int32_t* d_points, int n_points,
                                         double* d_cov_pp, const int32_t* d_cross, int n_cross,
                                         double* d_cov_pc, double rank_tol, double* d_ws, long long ws_len,
                                         int32_t* d_status, void* stream) {
  Launch La;
  if (int rc = make_launch(prob, 1, &La)) return rc;
  SLAM_REQUIRE(n_pairs >= 0 && n_points >= 0 && n_cross >= 0,
               "slam_ba_covariance_points: negative count (n_pairs %d, n_points %d, n_cross %d)", n_pairs,
               n_points, n_cross);
  SLAM_REQUIRE(n_pairs + (long long)n_points + n_cross >= 1, "slam_ba_covariance_points: nothing requested");
  SLAM_REQUIRE(std::isfinite(rank_tol) && rank_tol >= 0.0 && rank_tol < 1.0,
               "slam_ba_covariance_points: rank_tol %g must be finite and in [0, 1)", rank_tol);
  SLAM_REQUIRE(d_status != nullptr && (n_pairs == 0 || (d_pairs && d_cov)) &&
                   (n_points == 0 || (d_cov_pp && (d_points || n_points == prob->n_pts))) &&
                   (n_cross == 0 || (d_cross && d_cov_pc)),
               "slam_ba_covariance_points: null pointer (a null d_points needs n_points == n_pts = %d)",
               prob->n_pts);
  const CovLayout L(prob->n_cams);
  SLAM_REQUIRE(d_ws != nullptr && ws_len >= L.total,
               "slam_ba_covariance_points: workspace of %lld doubles, slam_ba_cov_workspace_len gives %lld",
               d_ws ? ws_len : 0ll, L.total);
  const CovRequest rq{d_pairs, n_pairs, d_cov, d_points, n_points, d_cov_pp, d_cross, n_cross, d_cov_pc, true};
  return cov_launch(La, rq, rank_tol, d_ws, d_status, slam::as_stream(stream));
}
