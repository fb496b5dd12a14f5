// BA, the one-workgroup camera solve k_solve_blk (9C <= kLdsMaxN: the local-BA
// window; larger systems: the tiled solves in ba_tiled.hip).
#include "ba_common.hpp"
#include "ba_epilogue.hpp"
#include "dpp_fmac.hpp"

namespace {

// ---------------------------------------------------------------- solve
// Reduced camera system S x = b, S SPD (damped).  Two solvers: k_solve_blk
// (one workgroup, whole system in LDS/registers) for the local-BA window
// (9C <= kLdsMaxN), and the tiled multi-workgroup Cholesky (k_tl3_flow, k_tl2_*) for
// larger systems.
constexpr int kSolveHdr = 32;   // doubles of LDS header in k_solve_blk

// -DSLAM_SOLVE_PROFILE: phase timestamps (wall_clock64, 100 MHz) of k_solve_blk
// into the spare LM state slots 12..15 (ns): load, eliminate, back-substitute,
// epilogue, and into slot 17 the assembly prologue of k_solve_blk<true> (a part
// of its load phase; ~0 in k_solve_blk<false>) (scripts/ba_solve_prof.py reads them).
#ifdef SLAM_SOLVE_PROFILE
#define SOLVE_PROF_T(i) uint64_t prof_t##i = wall_clock64()
#define SOLVE_PROF_END()                                                        \
  do {                                                                          \
    const uint64_t prof_e = wall_clock64();                                     \
    if (threadIdx.x == 0) {                                                     \
      p.state[12] = 10.0 * (double)(prof_t1 - prof_t0);                         \
      p.state[13] = 10.0 * (double)(prof_t2 - prof_t1);                         \
      p.state[14] = 10.0 * (double)(prof_t3 - prof_t2);                         \
      p.state[15] = 10.0 * (double)(prof_e - prof_t3);                          \
      p.state[17] = 10.0 * (double)(prof_ta - prof_t0);                         \
    }                                                                           \
  } while (0)
#else
#define SOLVE_PROF_T(i) (void)0
#define SOLVE_PROF_END() (void)0
#endif

// Small systems (9C <= kLdsMaxN, the local-BA window): blocked LDL^T with the
// trailing updates on the f64 matrix cores.
//
// The augmented matrix [S ; b^T] ((n+1) x n, b carried as row n so the
// elimination also performs the forward substitution) is kept as 16x16 f64
// MFMA accumulator tiles, lower tiles only, spread round-robin over the 4
// waves (<= 36 tiles for n <= 120, <= 9 per wave).  One block step per camera
// (9 columns):
//   (a) the owners of the 9 panel columns copy them to LDS;        barrier
//   (b) wave 0 factors the panel in registers, two rows per lane, pivot rows
//       broadcast with v_readlane (no LDS round trips, no barriers); it writes
//       W = -A_panel and L = A_panel D^-1 for the rows below the panel (zeros
//       elsewhere) and the final factor columns;                    barrier
//   (c) every wave updates its live tiles: T -= W_I L_J^T, 3 MFMAs
//       (v_mfma_f64_16x16x4_f64, K = 9 padded to 12) per tile.
// 2 barriers per camera instead of one per column.  Back substitution runs in
// wave 0 with x in registers (two rows per lane) and x_k broadcast by readlane.
constexpr int kBlkWG = 256;   // 4 waves, one per SIMD; <= 256 registers per lane (2 waves per SIMD)
constexpr int kBlkWaves = kBlkWG / 64;
constexpr int kTileMax = 9;   // lower 16x16 tiles per wave: 4 * 9 >= 36
constexpr int kPanelW = 9;    // columns per block step (one camera)
constexpr int kWLs = 13;      // W/L row stride: K = 9 padded to 3 MFMA steps of 4 (odd: no LDS bank conflicts)
static_assert(kLdsMaxN <= kBlkWG, "k_solve_blk prefetch assumes one element per thread");
static_assert(kBlkWaves * kTileMax >= ((kLdsMaxN + 16) / 16) * ((kLdsMaxN + 16) / 16 + 1) / 2,
              "kTileMax too small");

// 1/d from v_rcp_f64 refined by two Newton steps (full double precision, off
// the v_div_* sequence's long dependent chain)
__device__ __forceinline__ double rcp_f64(double d) {
  double r = __builtin_amdgcn_rcp(d);
  double e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-d, r, 1.0);
  return __builtin_fma(r, e, r);
}

__device__ __forceinline__ double readlane_d(double v, int lane) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// LDS layout of k_solve_blk (doubles, after the kSolveHdr header)
struct BlkLds {
  int n16;        // rows rounded up to a tile multiple (>= n + 1)
  int pn, wl, ll, lf, dd, yy, xx, ep, total;
  __host__ __device__ explicit BlkLds(int n) {
    n16 = ((n + 1 + 15) / 16) * 16;
    pn = kSolveHdr;                       // [n16][kPanelW] panel copy
    wl = pn + n16 * kPanelW;              // [n16][kWLs] W = -A_panel (rows below the panel)
    ll = wl + n16 * kWLs;                 // [n16][kWLs] L = A_panel D^-1
    lf = ll + n16 * kWLs;                 // [n(n-1)/2] factor L, packed by rows
    dd = lf + ((n * (n - 1) / 2 + 1) & ~1);  // [n] D
    yy = dd + ((n + 1) & ~1);             // [n] y = L^-1 b
    xx = yy + ((n + 1) & ~1);             // [n] solution
    ep = xx + ((n + 1) & ~1);             // [5][n] b, g, diagU, live cameras, cost partials
    total = ep + 5 * ((n + 1) & ~1);
  }
};

// -DSLAM_SOLVE_TRACE: s_memtime of problem 0's thread 0 at the points of each
// block step (rows 0..17; 18, 19: after the loop and the load); slam_solve_trace
// reads them (scripts/solve_trace.py).
#ifdef SLAM_SOLVE_TRACE
__device__ unsigned long long g_solve_trace[20][6];
#define SOLVE_TR(step, i)                                                        \
  do {                                                                           \
    if (threadIdx.x == 0 && blockIdx.y == 0 && (step) < 20)                      \
      g_solve_trace[step][i] = __builtin_amdgcn_s_memtime();                     \
  } while (0)
#else
#define SOLVE_TR(step, i) (void)0
#endif

// ---------------------------------------------------------------- assembly prologue
// k_solve_blk<true> sums the window's partial rows itself, on its own 4 waves,
// and gives what k_assemble gives bit for bit.  k_assemble's order is that of
// rows_sum<1024, 8, false, kCPart> (ba.hip): virtual lane (part k, column e) of
// a 1024-lane workgroup, nparts = 1024 / n, holds 8 accumulators a[u] (from
// +0.0) over the rows rb + k + (u + 8 m) nparts, m = 0, 1, ... (its unrolled
// trips and its remainder loop deal the rows to the accumulators alike), folds
// them with the fixed tree pair_sum<8>, and the parts are added in order
// k = 0, 1, ... onto +0.0.  Here one real lane walks all the parts of its
// column in that order, so no LDS carries the parts.
constexpr int kAsmVirt = 1024;  // k_assemble's workgroup (SLAM_ASM_WG of ba.hip)
constexpr int kAsmNF = 8;       // its accumulators per virtual lane
constexpr int kAsmGrp = 3;      // parts a lane walks together on the deep path (divides 9 and 12)

template <int N>  // (a[0] + a[1]) + (a[2] + a[3]), ...: ba.hip's pair_sum
__device__ __forceinline__ double asm_pair_sum(const double* a) {
  if constexpr (N == 1) return a[0];
  else return asm_pair_sum<N / 2>(a) + asm_pair_sum<N / 2>(a + N / 2);
}

// Column sums of the N-wide rows [rb, re) of part for the columns lane and
// lane + 64 (the second clamped to N - 1: its spare lanes repeat the last
// column and drop the result), in the virtual order above.  Up to HOIST rows
// per part (all local-BA windows of the tracker) every load of both columns is
// issued before the first add; the rows a part does not have enter as +0.0,
// which changes no bit (an accumulator starts at +0.0 and so is never -0.0,
// and x + +0.0 == x for every other x).  Deeper runs walk kAsmGrp parts at a
// time through k_assemble's 8-deep trips.
template <int N, int HOIST>
__device__ __forceinline__ void virt_rows_sum2(const double* __restrict__ part, int stride, int rb,
                                               int re, int lane, double& o0, double& o1) {
  constexpr int P = kAsmVirt / N;
  static_assert(HOIST <= kAsmNF, "hoisted rows of a part: one accumulator each");
  const double* q0 = part + (size_t)rb * stride + lane;
  const double* q1 = part + (size_t)rb * stride + min(lane + 64, N - 1);
  const int R = re - rb;  // uniform
  double v0 = 0.0, v1 = 0.0;
  if (R <= HOIST * P) {
    double x0[HOIST * P], x1[HOIST * P];
#pragma unroll
    for (int i = 0; i < HOIST * P; ++i) {
      x0[i] = 0.0;
      x1[i] = 0.0;
      if (i < R) {
        x0[i] = q0[(size_t)i * stride];
        x1[i] = q1[(size_t)i * stride];
      }
    }
#pragma unroll
    for (int k = 0; k < P; ++k) {
      double a0[kAsmNF] = {}, a1[kAsmNF] = {};
#pragma unroll
      for (int u = 0; u < HOIST; ++u) {
        a0[u] += x0[k + u * P];
        a1[u] += x1[k + u * P];
      }
      v0 += asm_pair_sum<kAsmNF>(a0);
      v1 += asm_pair_sum<kAsmNF>(a1);
    }
  } else {
    // kAsmGrp parts at a time, trip by trip: the 8 rows of a trip of each part
    // (k_assemble's unrolled trip; its remainder is the last, partial trip with
    // the same deal of rows to accumulators) are loaded before they are added
    static_assert(P % kAsmGrp == 0, "parts walked in groups");
    const int trips = ((R + P - 1) / P + kAsmNF - 1) / kAsmNF;
#pragma unroll 1
    for (int k0 = 0; k0 < P; k0 += kAsmGrp) {
      double a0[kAsmGrp][kAsmNF] = {}, a1[kAsmGrp][kAsmNF] = {};
#pragma unroll 1
      for (int m = 0; m < trips; ++m) {
        double y0[kAsmGrp][kAsmNF], y1[kAsmGrp][kAsmNF];
#pragma unroll
        for (int g = 0; g < kAsmGrp; ++g)
#pragma unroll
          for (int u = 0; u < kAsmNF; ++u) {
            const int r = k0 + g + (u + kAsmNF * m) * P;
            y0[g][u] = 0.0;
            y1[g][u] = 0.0;
            if (r < R) {
              y0[g][u] = q0[(size_t)r * stride];
              y1[g][u] = q1[(size_t)r * stride];
            }
          }
#pragma unroll
        for (int g = 0; g < kAsmGrp; ++g)
#pragma unroll
          for (int u = 0; u < kAsmNF; ++u) {
            a0[g][u] += y0[g][u];
            a1[g][u] += y1[g][u];
          }
      }
#pragma unroll
      for (int g = 0; g < kAsmGrp; ++g) {
        v0 += asm_pair_sum<kAsmNF>(a0[g]);
        v1 += asm_pair_sum<kAsmNF>(a1[g]);
      }
    }
  }
  o0 = v0;
  o1 = v1;
}

// The staged tiles (all lower 16x16 tiles, 256 doubles each, from Pn on) end
// before Dd for every window size.
constexpr bool asm_stage_fits() {
  for (int c = 1; 9 * c <= kLdsMaxN; ++c) {
    const int n = 9 * c, n16 = ((n + 1 + 15) / 16) * 16, nt = n16 / 16;
    if (nt * (nt + 1) / 2 * 256 > n16 * (kPanelW + 2 * kWLs) + n * (n - 1) / 2) return false;
  }
  return true;
}
static_assert(asm_stage_fits(), "k_solve_blk<true>: the tile staging overruns Pn / WL / LL / LF");

// What k_assemble writes into sys (dense layout: S with both mirrored entries
// of an off-diagonal block, b, g, diag U, per-camera cost; the write-out
// statements are its statements), one wave per block, blocks dealt round-robin
// over the 4 waves; lane l holds elements l and 64 + l of the block's 81 (of the
// camera row's 109).  The same values go to stg (the lower tiles, tile
// I (I + 1) / 2 + J at 256 doubles, row-major 16 x 16) and to Eb (b, g, diag U
// at 0, n2, 2 n2; cost at 4 n2), from which the solve continues.
__device__ __forceinline__ void asm_prologue(const slam_ba_problem& p, double* stg, double* Eb,
                                             int n2, int wid, int lane) {
  const int C9 = 9 * p.n_cams;
  double* S = p.sys;
  double* bvec = S + sys_vec_off(p.n_cams, p.n_blocks);
  double* gvec = bvec + C9;
  double* diagU = gvec + C9;
  double* costc = diagU + C9;
  auto put = [&](int row, int col, double v) {
    S[(size_t)row * C9 + col] = v;
    const int I = row >> 4, J = col >> 4;
    if (I >= J) stg[(I * (I + 1) / 2 + J) * 256 + (row & 15) * 16 + (col & 15)] = v;
  };
  for (int blk = wid; blk < p.n_blocks; blk += kBlkWaves) {  // uniform per wave
    const int c1 = p.blocks[2 * blk], c2 = p.blocks[2 * blk + 1];
    const bool diag = c1 == c2;
    const int bb = p.blk_bslot_ptr[blk], be = p.blk_bslot_ptr[blk + 1];
    const int t0 = lane, t1 = min(lane + 64, 80);
    const bool has1 = lane + 64 < 81;
    const int i0 = t0 / 9, j0 = t0 - 9 * i0, i1 = t1 / 9, j1 = t1 - 9 * i1;
    if (!diag && be == bb) {  // a block without partial rows: -sum of nothing
      put(9 * c1 + i0, 9 * c2 + j0, -0.0);
      put(9 * c2 + j0, 9 * c1 + i0, -0.0);
      if (has1) {
        put(9 * c1 + i1, 9 * c2 + j1, -0.0);
        put(9 * c2 + j1, 9 * c1 + i1, -0.0);
      }
      continue;
    }
    double sh0 = 0.0, sh1 = 0.0, sb0 = 0.0, sb1 = 0.0;
    if (diag)
      virt_rows_sum2<109, 4>(p.cpart, kCPart, p.cam_cslot_ptr[c1], p.cam_cslot_ptr[c1 + 1], lane, sh0, sh1);
    if (!diag || be > bb) virt_rows_sum2<81, 3>(p.bpart, 81, bb, be, lane, sb0, sb1);
    if (diag) {
      // sb[9 j + i] of the other lanes, sh[90 + t] beside sh[81 + t]
      const int s0 = 9 * j0 + i0, s1 = 9 * j1 + i1;
      const double a0 = __shfl(sb0, s0 & 63, 64), b0 = __shfl(sb1, s0 & 63, 64);
      const double a1 = __shfl(sb0, s1 & 63, 64), b1 = __shfl(sb1, s1 & 63, 64);
      const double sbT0 = s0 < 64 ? a0 : b0, sbT1 = s1 < 64 ? a1 : b1;
      const double shu = __shfl(sh1, (lane + 9) & 63, 64);
      put(9 * c1 + i0, 9 * c1 + j0, sh0 - (sb0 + sbT0));
      if (has1) put(9 * c1 + i1, 9 * c1 + j1, sh1 - (sb1 + sbT1));
      const int e = lane + 64;
      if (e >= 81 && e < 90) {
        const int q = 9 * c1 + e - 81;
        const double gv = -sh1, bv = -sh1 - shu;
        gvec[q] = gv;
        bvec[q] = bv;
        Eb[n2 + q] = gv;
        Eb[q] = bv;
      }
      if (e >= 99 && e < 108) {
        diagU[9 * c1 + e - 99] = sh1;
        Eb[2 * n2 + 9 * c1 + e - 99] = sh1;
      }
      if (e == 108) {
        costc[c1] = sh1;
        Eb[4 * n2 + c1] = sh1;
      }
    } else {
      put(9 * c1 + i0, 9 * c2 + j0, -sb0);
      put(9 * c2 + j0, 9 * c1 + i0, -sb0);
      if (has1) {
        put(9 * c1 + i1, 9 * c2 + j1, -sb1);
        put(9 * c2 + j1, 9 * c1 + i1, -sb1);
      }
    }
  }
}

// ASM: the workgroup first assembles its window's sys from the partial rows
// (asm_prologue above; no k_assemble launch before it) and takes the tile
// values and b, g, diag U, cost from LDS instead of from sys.
template <bool ASM>
__global__ __launch_bounds__(kBlkWG) __attribute__((amdgpu_waves_per_eu(2))) void k_solve_blk(BaBatch bat) {
  BA_PROB(bat);
  lm_wave_priority();
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* red = lds;
  int* fail_p = reinterpret_cast<int*>(lds + 16);
  const int n = 9 * p.n_cams;
  const BlkLds g(n);
  double* Pn = lds + g.pn;
  double* WL = lds + g.wl;
  double* LL = lds + g.ll;
  double* LF = lds + g.lf;
  double* Dd = lds + g.dd;
  double* Yy = lds + g.yy;
  double* X = lds + g.xx;
  const double* S = p.sys;
  const double* bvec = S + (size_t)n * n;
  const double* diagU = bvec + 2 * n;
  const double lam = p.state[SLAM_BA_ST_LAMBDA];
  const int t = threadIdx.x, lane = t & 63;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
  const int NT = g.n16 / 16, NL = NT * (NT + 1) / 2;
  SOLVE_PROF_T(0);
  SOLVE_TR(19, 1);
  const int n2 = (n + 1) & ~1;
  if (t == 0) *fail_p = 0;
  if constexpr (!ASM)
    for (int i = t; i < 2 * g.n16 * kWLs; i += kBlkWG) WL[i] = 0.0;  // WL and LL
  if constexpr (ASM) {
    // the sums go to sys (an output only: never read back here), to the tile
    // staging in Pn..LF (dead until the first panel) and to Eb (below)
    double* Ea = lds + g.ep;
    asm_prologue(p, Pn, Ea, n2, wid, lane);
    const double cv = p.cams[cur_of(p.state)][min(t, n - 1)];
    if (t < n) Ea[3 * n2 + t] = cv;
    __syncthreads();  // staged tiles, b, g, diag U, cameras, cost
  }
  SOLVE_PROF_T(a);
  // this wave's tiles: tl = wid + 4 s -> (I, J), I >= J.  All S loads are
  // issued unconditionally (clamped addresses) before any is used.
  int tI[kTileMax], tJ[kTileMax];
  d4 acc[kTileMax];
#pragma unroll
  for (int s = 0; s < kTileMax; ++s) {
    const int tl = wid + kBlkWaves * s;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= tl) ++I;
    tI[s] = tl < NL ? I : -1;
    tJ[s] = tl < NL ? tl - I * (I + 1) / 2 : -1;
    const int col = min(max(tJ[s], 0) * 16 + (lane & 15), n - 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = min(max(tI[s], 0) * 16 + (lane >> 4) + 4 * q, n - 1);
      if constexpr (ASM) acc[s][q] = Pn[(tl < NL ? tl : 0) * 256 + ((lane >> 4) + 4 * q) * 16 + (lane & 15)];
      else acc[s][q] = S[(size_t)row * n + col];
    }
  }
  double* Eb = lds + g.ep;  // prefetch: b, g, diagU, live cameras, cost partials
  if constexpr (ASM) {
    __syncthreads();  // the staging is dead: WL / LL may be cleared, Pn written
    for (int i = t; i < 2 * g.n16 * kWLs; i += kBlkWG) WL[i] = 0.0;  // WL and LL
  } else {
    const double* src[5] = {bvec, bvec + n, diagU, p.cams[cur_of(p.state)], diagU + n};
    const int len[5] = {n, n, n, n, p.n_cams};
    double v[5];  // n <= kLdsMaxN < kBlkWG: one element per thread, loads issued together
#pragma unroll
    for (int a = 0; a < 5; ++a) v[a] = src[a][min(t, len[a] - 1)];
#pragma unroll
    for (int a = 0; a < 5; ++a)
      if (t < len[a]) Eb[a * n2 + t] = v[a];
    __syncthreads();  // prefetched b and diagU
  }
#pragma unroll
  for (int s = 0; s < kTileMax; ++s) {
    const int col = tJ[s] * 16 + (lane & 15);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = tI[s] * 16 + (lane >> 4) + 4 * q;
      double a = acc[s][q];
      if (row == col) a += lam * clampd(Eb[2 * n2 + col]);
      if (row == n) a = Eb[min(col, n - 1)];
      if (tI[s] < 0 || col >= n || row > n) a = 0.0;
      acc[s][q] = a;
    }
  }
  SOLVE_PROF_T(1);
  bool ok = true;
  SOLVE_TR(19, 0);
  for (int c0 = 0; c0 < n; c0 += kPanelW) {
    SOLVE_TR(c0 / kPanelW, 0);
    // (a) panel columns [c0, c0 + 9), rows c0..n -> Pn[row - c0][col - c0]
#pragma unroll
    for (int s = 0; s < kTileMax; ++s) {
      if (tI[s] < 0 || tJ[s] * 16 + 15 < c0 || tJ[s] * 16 >= c0 + kPanelW || tI[s] * 16 + 15 < c0)
        continue;  // uniform per wave
      const int col = tJ[s] * 16 + (lane & 15);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = tI[s] * 16 + (lane >> 4) + 4 * q;
        if (col >= c0 && col < c0 + kPanelW && col <= row && row >= c0 && row <= n)
          Pn[(row - c0) * kPanelW + (col - c0)] = acc[s][q];
      }
    }
    __syncthreads();
    SOLVE_TR(c0 / kPanelW, 1);
    // (b) panel factorisation, one panel row per lane: lanes 0..8 of every
    // participating wave hold the 9 pivot rows r = c0 + m (lower entries),
    // lanes 9..63 of wave w the rows c0 + 9 + 55 w + (lane - 9) (the rhs row n
    // included).  Right-looking: at step j the pivot d_j and the column-j
    // entries of the pivot rows are broadcast with v_readlane, and every lane
    // eliminates its own row (u_i -= (u_j / d_j) A(c0+i, c0+j)).  Afterwards
    // u_j is the partially eliminated entry A^{(j)}(r, c0+j), L(r, j) = u_j/d_j.
    // (Was: every lane factored the whole 9x9 block redundantly, ~3x the
    // VALU work of this form.)
    // Every 16-lane DPP row of a participating wave holds a copy of the 9 pivot
    // rows (lanes 0..8 of the row) and 7 rows below the panel (lanes 9..15), so
    // the pivot entries reach the other lanes as DPP row_newbcast operands
    // (no v_readlane -> SGPR hop in the pivot chain).  28 rows below per wave:
    // 4 waves cover 9C + 1 - 9 <= 112 rows.
    constexpr int kRowsBelow = 16 - kPanelW;              // per DPP row
    const int nbelow = n + 1 - c0 - kPanelW;             // rows below the panel, rhs included
    const int nw = max(1, (nbelow + 4 * kRowsBelow - 1) / (4 * kRowsBelow));  // uniform
    if (wid < nw) {
      const int rl = lane & 15, rg = lane >> 4;
      const bool piv = rl < kPanelW;
      const int r = piv ? c0 + rl
                        : c0 + kPanelW + 4 * kRowsBelow * wid + kRowsBelow * rg + (rl - kPanelW);
      const bool valid = r <= n;
      const double* pr = Pn + (r - c0) * kPanelW;
      double u[kPanelW];
#pragma unroll
      for (int j = 0; j < kPanelW; ++j) u[j] = valid && (!piv || j <= rl) ? pr[j] : 0.0;
      double Dinv[kPanelW];
      bool bad = false;
      static_for<0, kPanelW>([&](auto J) {
        constexpr int j = decltype(J)::value;
        const double d = bcast16<j>(u[j]);
        bad |= !(d > 0.0) || !isfinite(d);
        Dinv[j] = rcp_f64(d);
        const double l = u[j] * Dinv[j];
        if constexpr (j + 1 < kPanelW) u[j + 1] = __builtin_fma(-l, bcast16<j + 1>(u[j]), u[j + 1]);
        // u[i] += bcast_i(u[j]) * -l for i = j+2..8: column j's updates after the
        // next pivot's entry, which stays in compiler code (dpp_fmac.hpp)
        static_assert(kPanelW == 9, "the BcastFmaTail ranges of dpp_fmac.hpp end at row 8");
        BcastFmaTail<j + 2, kPanelW - 1>::run(u, u[j], -l);
      });
      // stores grouped so that each lane class takes one exec-mask region
      if (valid && ((wid == 0 && rg == 0) || !piv)) {
        double* wl = WL + r * kWLs;
        double* ll = LL + r * kWLs;
        double* lf = LF + r * (r - 1) / 2 + c0;
        double lj[kPanelW];
#pragma unroll
        for (int j = 0; j < kPanelW; ++j) {
          lj[j] = u[j] * Dinv[j];
          wl[j] = -u[j];
          ll[j] = lj[j];
        }
        if (r == n) {
#pragma unroll
          for (int j = 0; j < kPanelW; ++j) Yy[c0 + j] = u[j];
        } else if (!piv) {
#pragma unroll
          for (int j = 0; j < kPanelW; ++j) lf[j] = lj[j];
        } else {
          // pivot row m = lane: D_m and the lower part L(r, c0 + j), j < m
          double dm = u[0];
#pragma unroll
          for (int j = 1; j < kPanelW; ++j) dm = j == rl ? u[j] : dm;
          Dd[r] = dm;
#pragma unroll
          for (int j = 0; j < kPanelW - 1; ++j)
            if (j < rl) lf[j] = lj[j];
        }
      }
      if (wid == 0 && lane == 0 && bad) *fail_p = 1;
    }
    SOLVE_TR(c0 / kPanelW, 2);
    __syncthreads();
    SOLVE_TR(c0 / kPanelW, 3);
    if (*fail_p) {
      ok = false;
      break;
    }
    // (c) trailing update of the tiles right of / below the panel, tile by
    // tile (6 operand loads, then its 3 MFMAs; each tile's sum in the same kk
    // order).  Loading every live tile's operands first held ~100 more
    // registers (317 per lane: one wave per SIMD, so a solve workgroup waited
    // for a whole idle CU beside ORB); at 210 (two waves per SIMD) the batched
    // local-BA stage in the tracking bench drops 3.1 -> 2.75 ms per step
    // (profiles/r4/solve_lowreg_ab/ at git f26058c)
    const int tr = c0 + kPanelW;
#pragma unroll
    for (int s = 0; s < kTileMax; ++s) {
      if (!(tI[s] >= 0 && tJ[s] * 16 + 15 >= tr)) continue;  // uniform (I >= J)
      const double* wrow = WL + (tI[s] * 16 + (lane & 15)) * kWLs + (lane >> 4);
      const double* lrow = LL + (tJ[s] * 16 + (lane & 15)) * kWLs + (lane >> 4);
      double wa[3], lb[3];
#pragma unroll
      for (int kk = 0; kk < 3; ++kk) {
        wa[kk] = wrow[4 * kk];
        lb[kk] = lrow[4 * kk];
      }
#pragma unroll
      for (int kk = 0; kk < 3; ++kk)
        acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[kk], lb[kk], acc[s], 0, 0, 0);
    }
#ifdef SLAM_SOLVE_TRACE
    if (threadIdx.x == 0) {
      double chk = acc[0][0];
      __asm__ volatile("" : "+v"(chk));
      acc[0][0] = chk;
    }
    SOLVE_TR(c0 / kPanelW, 4);
#endif
  }
  SOLVE_PROF_T(2);
  SOLVE_TR(18, 0);
  if (ok && wid == 0) {
    // z = D^-1 y, then L^T x = z from the bottom; lane l holds rows l, l + 64.
    // Step k: x_i -= L(k, i) x_k for i < k, x_k broadcast by v_readlane.  Rows
    // k >= 64 update every x0 (i = lane < 64 <= k, no mask) and the x1 rows
    // below k; rows k < 64 update x0 only.  The L rows of kBackU steps are
    // loaded (clamped, then masked by a select) ahead of the dependent chain.
    double x0 = lane < n ? Yy[lane] / Dd[lane] : 0.0;
    double x1 = lane + 64 < n ? Yy[lane + 64] / Dd[lane + 64] : 0.0;
    constexpr int kBackU = 8;
    int k = n - 1;
    for (; k - kBackU + 1 >= 64; k -= kBackU) {
      double l0[kBackU], l1[kBackU];
#pragma unroll
      for (int u = 0; u < kBackU; ++u) {
        const int kk = k - u;
        const double* Lk = LF + kk * (kk - 1) / 2;
        l0[u] = Lk[lane];
        const double v = Lk[min(lane + 64, kk - 1)];
        l1[u] = lane + 64 < kk ? v : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kBackU; ++u) {
        const double xk = readlane_d(x1, k - u - 64);
        x0 = __builtin_fma(-l0[u], xk, x0);
        x1 = __builtin_fma(-l1[u], xk, x1);
      }
    }
    for (; k >= 64; --k) {
      const double* Lk = LF + k * (k - 1) / 2;
      const double v = Lk[min(lane + 64, k - 1)];
      const double xk = readlane_d(x1, k - 64);
      x0 = __builtin_fma(-Lk[lane], xk, x0);
      x1 = __builtin_fma(-(lane + 64 < k ? v : 0.0), xk, x1);
    }
    for (; k - kBackU + 1 >= 1; k -= kBackU) {
      double l0[kBackU];
#pragma unroll
      for (int u = 0; u < kBackU; ++u) {
        const int kk = k - u;
        const double v = LF[kk * (kk - 1) / 2 + min(lane, kk - 1)];
        l0[u] = lane < kk ? v : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kBackU; ++u) x0 = __builtin_fma(-l0[u], readlane_d(x0, k - u), x0);
    }
    for (; k >= 1; --k) {
      const double v = LF[k * (k - 1) / 2 + min(lane, k - 1)];
      x0 = __builtin_fma(-(lane < k ? v : 0.0), readlane_d(x0, k), x0);
    }
    if (lane < n) X[lane] = x0;
    if (lane + 64 < n) X[lane + 64] = x1;
  }
  __syncthreads();
  SOLVE_PROF_T(3);
  SOLVE_TR(18, 1);
  solve_epilogue(p, X, ok, red, EpiSrc{Eb + n2, Eb + 2 * n2, Eb + 3 * n2, Eb + 4 * n2});
  SOLVE_PROF_END();
  SOLVE_TR(18, 2);
}

}  // namespace

size_t slam::solve_blk_lds(int n_cams) { return sizeof(double) * BlkLds(9 * n_cams).total; }

int slam::launch_solve_blk(const Launch& L, hipStream_t s) {
  if (L.fused) k_solve_blk<true><<<dim3(1, L.n), kBlkWG, L.solve_lds, s>>>(L.b);
  else k_solve_blk<false><<<dim3(1, L.n), kBlkWG, L.solve_lds, s>>>(L.b);
  SLAM_LAUNCHED("k_solve_blk");
  return SLAM_OK;
}

#ifdef SLAM_SOLVE_TRACE
extern "C" int slam_solve_trace(unsigned long long* out) {
  SLAM_HIP(hipDeviceSynchronize());
  SLAM_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_solve_trace), 20 * 6 * sizeof(unsigned long long)));
  return SLAM_OK;
}
#endif
