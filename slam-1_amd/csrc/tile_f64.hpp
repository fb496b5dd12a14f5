// The 64x64 f64 tile operations shared by the tiled solvers: the tiled BA solve
// (ba_tiled.hip), the camera covariance (ba_cov.hip) and the pose graph's
// skyline factor (posegraph_se3.hip).  Fragment-ordered LDS images of a tile as
// MFMA operands, the tile products on v_mfma_f64_16x16x4_f64, the factor +
// inverse of a diagonal tile (tile_chol_inv_blk), and the three steps of a
// tiled solve written once (tile_panel, tile_update, tile_back, at the end).
// Every function is inlined into its kernel and nothing here is a kernel.  The
// three steps declare their own LDS (__shared__: tile_panel 96 KB + a flag,
// tile_update 64 KB and 2 KB with a right-hand side, tile_back 2.5 KB), so a
// kernel that calls one has that much LDS; nothing else has storage outside
// SLAM_FLOW_PROFILE.
#pragma once

#include "ba_common.hpp"
#include "dpp_fmac.hpp"

namespace {

#ifndef SLAM_TL_PADSKIP
#define SLAM_TL_PADSKIP 1  // the tile factor skips the pivot chain of padding blocks
#endif
constexpr int kTB = 64;        // tile edge
constexpr int kTlWG = 256;     // 4 waves: wave w owns rows 16w..16w+15 of a tile

// fragment-ordered LDS image of a 64x64 tile: the MFMA operand of sub-tile s,
// k-step kk is 64 consecutive doubles (lane l: row 16s + (l & 15), col 4kk + (l >> 4))
__device__ __forceinline__ int frag_idx(int r, int c) {
  return ((((r >> 4) << 4) + (c >> 2)) << 6) + (r & 15) + ((c & 3) << 4);
}

__device__ __forceinline__ void tile_to_frag(const double* __restrict__ g, int ld, double* f,
                                             int w = threadIdx.x >> 6, int nw = kTlWG / 64) {
  // wave w of nw writes fragments (s, kk) = w, w + nw, ...: 64 consecutive doubles
  // per fragment (conflict-free LDS stores); the global reads are 16 rows x 32 B
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, c = lane >> 4;
  // 16 loads in flight per lane before their LDS stores
  for (int f0 = w; f0 < 64; f0 += 16 * nw) {
    double tmp[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int fi = f0 + q * nw;
      tmp[q] = fi < 64 ? g[(size_t)(16 * (fi >> 4) + r) * ld + 4 * (fi & 15) + c] : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int fi = f0 + q * nw;
      if (fi < 64) f[(fi << 6) + lane] = tmp[q];
    }
  }
}

// acc[s] (wave w) = rows 16w.., cols 16s.. of X Y^T with Y LOWER triangular
// (L_kk^-1): column block s takes only the k-steps kk <= 4s + 3 (Y's entries
// past them are exact zeros), 40 of the 64 MFMAs -- the same sums.
__device__ __forceinline__ void gemm_xyT_lowY(const double* Xf, const double* Yf, d4 acc[4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
  static_for<0, 16>([&](auto K) {
    constexpr int kk = decltype(K)::value;
    const double a = Xf[((w * 16 + kk) << 6) + lane];
    static_for<kk / 4, 4>([&](auto S) {
      constexpr int s = decltype(S)::value;
      acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Yf[((s * 16 + kk) << 6) + lane], acc[s], 0, 0, 0);
    });
  });
}

// Blocked factor + inverse of the 64x64 diagonal tile (4 x 4 blocks of 16):
// per block column p, wave 0 factors the 16x16 diagonal block in registers
// (lane i = row i, pivots and column entries broadcast by DPP row_newbcast)
// and inverts it (lane c = column c of L_pp^-1); the panel L_ip = A_ip L_pp^-T
// and the trailing update A_ij -= L_ip L_jp^T run on the f64 matrix cores
// (16x16x4), one block per wave, for p = 0, 1 (workgroup barriers between);
// block columns 2 and 3 (L_32, A_33 and both factors) are wave 0's chain
// alone.  L^-1's off-diagonal blocks X_ip = -X_ii sum_{k=p}^{i-1} L_ik X_kp
// are formed by waves 1-3 beside that chain as their inputs appear (round 5:
// X_10 during block 2's factor, X_21 / X_20 and the sums T_3p during block
// 3's, the last three products X_3p = -X_33 T_3p once X_33 is out), so after
// the last pivot only one 16x16 product per wave is left (the assembly after
// the factor was 2.2 us of 13.0 per tile; 0.44 now).  M: LDS [64][65] (A, then
// L's off-diagonal blocks), Xb: LDS [10][16][17] (lower blocks of L^-1), Tb:
// LDS [3][16][17] scratch + six int flags (the wave-to-wave hand-offs of
// L_10 .. L_32, right after the scratch).  Every wave must call
// it; returns false (uniform) on a non-positive or non-finite pivot.
constexpr int kMS = 65;   // row stride of M (odd: MFMA operand reads spread over banks)
constexpr int kBS17 = 17; // row stride of a 16x16 block
__device__ __forceinline__ int blk_id(int i, int j) { return i * (i + 1) / 2 + j; }

// C (+)= X Y^T (16x16 blocks, strides sx / sy); a_neg negates the product
__device__ __forceinline__ d4 mm16_xyT(const double* X, int sx, const double* Y, int sy, d4 acc,
                                       bool a_neg) {
  const int l = threadIdx.x & 63;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const double a = X[(l & 15) * sx + 4 * kk + (l >> 4)];
    const double b = Y[(l & 15) * sy + 4 * kk + (l >> 4)];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a_neg ? -a : a, b, acc, 0, 0, 0);
  }
  return acc;
}
// C (+)= X Y (16x16 blocks)
__device__ __forceinline__ d4 mm16_xy(const double* X, int sx, const double* Y, int sy, d4 acc,
                                      bool a_neg) {
  const int l = threadIdx.x & 63;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const double a = X[(l & 15) * sx + 4 * kk + (l >> 4)];
    const double b = Y[(4 * kk + (l >> 4)) * sy + (l & 15)];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a_neg ? -a : a, b, acc, 0, 0, 0);
  }
  return acc;
}
__device__ __forceinline__ void st16(double* C, int sc, d4 acc) {
  const int l = threadIdx.x & 63;
#pragma unroll
  for (int r = 0; r < 4; ++r) C[((l >> 4) + 4 * r) * sc + (l & 15)] = acc[r];
}
__device__ __forceinline__ d4 ld16(const double* C, int sc) {
  const int l = threadIdx.x & 63;
  d4 acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = C[((l >> 4) + 4 * r) * sc + (l & 15)];
  return acc;
}

// -DSLAM_FLOW_PROFILE: wall clock at the steps of workgroup 0's tile factor
// (slam_flow_fac_stamps, scripts/flow_prof.py)
#ifdef SLAM_FLOW_PROFILE
__device__ unsigned long long g_flow_fac[16];
#define FAC_T(i)                                                    \
  do {                                                              \
    if (blockIdx.x == 0 && threadIdx.x == 0) g_flow_fac[i] = wall_clock64(); \
  } while (0)
#else
#define FAC_T(i) (void)0
#endif
// LDS written by this wave visible to its own later reads (no other wave involved)
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Wave 0's part of block column p: the 16x16 diagonal block of M factored in
// registers and inverted (X_pp = L_pp^-1 into Xb); `ok` cleared on a
// non-positive or non-finite pivot.
__device__ __forceinline__ void blk_factor_w0(double* M, double* Xb, int p, bool& ok) {
  const int l = threadIdx.x & 63;
  const int i = l & 15;
  double v[16], rj[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) v[c] = c <= i ? M[(16 * p + i) * kMS + 16 * p + c] : 0.0;
  // Pivot chain: d_j -> rsq + 2 Newton steps -> p = v_j r (row i's L_ij for
  // i > j) -> lane j+1's own update d_{j+1} = v_{j+1} - p^2 -> broadcast.  The
  // broadcasts of column j to the other rows read p from rows m > j only, so
  // they need no select; the whole-row update of column j (fused DPP FMAs)
  // is off the chain.  Same operations as the plain right-looking form.
  double dn = bcast16<0>(v[0]);
  static_for<0, 16>([&](auto J) {
    constexpr int j = decltype(J)::value;
    const double djj = dn;
    ok = ok && djj > 0.0 && djj < INFINITY;
    double r = __builtin_amdgcn_rsq(djj);
    const double h = 0.5 * djj;
    r = r * __builtin_fma(-h * r, r, 1.5);
    r = r * __builtin_fma(-h * r, r, 1.5);
    rj[j] = r;
    const double pj = v[j] * r;
    if constexpr (j + 1 < 16) dn = bcast16<j + 1>(__builtin_fma(-pj, pj, v[j + 1]));
    const double lij = i > j ? pj : (i == j ? djj * r : 0.0);
    v[j] = lij;
    BcastFmaTail<j + 1, 15>::run(v, -pj, lij);
  });
  FAC_T(2 + 3 * p);  // (profiling build: wave 0's pivots of block p done)
  // column c = lane of L_pp^-1: x_c = 1 / l_cc, x_i = -(sum_{k<i} l_ik x_k) / l_ii
  // (column-oriented: once x_k is known, every later row's sum takes its
  // term -- the same k order per sum as the row form, a 16-step chain
  // instead of 120 dependent FMAs); l_ik = lane ii's v[k], by row_newbcast.
  // The sum of row c starts at -1 so that x_k = -s_k / l_kk holds for every
  // k >= c with no select on the chain (x_c = 1 / l_cc exactly; the rows
  // above c carry signed zeros, written as 0 below)
  const int c = l & 15;
  double x[16], sacc[16];
#pragma unroll
  for (int ii = 0; ii < 16; ++ii) sacc[ii] = ii == c ? -1.0 : 0.0;
  static_for<0, 16>([&](auto K) {
    constexpr int k = decltype(K)::value;
    x[k] = -sacc[k] * rj[k];
    BcastFmaTail<k + 1, 15>::run(sacc, v[k], x[k]);
  });
  if (l < 16) {
    double* X = Xb + blk_id(p, p) * 16 * kBS17;
#pragma unroll
    for (int ii = 0; ii < 16; ++ii) X[ii * kBS17 + c] = ii < c ? 0.0 : x[ii];
  }
}

// nb: the tile's 16-row blocks that hold rows of S (ba.tl_schedule: a tile of
// c whole cameras has 9c rows, the rest padding with a unit diagonal and no
// coupling); wave 0 skips the pivot chain of every block p >= nb, whose factor
// and inverse are the identity (X_pp = I written directly), so a 45-row tile
// runs three 16x16 factors instead of four.  Waves 1-3 still form the blocks of
// L / L^-1 in the padding rows (exact zeros) beside the chain.
__device__ __forceinline__ void blk_identity_w0(double* Xb, int p) {
  const int l = threadIdx.x & 63;
  if (l < 16) {
    double* X = Xb + blk_id(p, p) * 16 * kBS17;
#pragma unroll
    for (int ii = 0; ii < 16; ++ii) X[ii * kBS17 + l] = ii == l ? 1.0 : 0.0;
  }
}

// The tile factor (described above kMS).  Akk == nullptr: the tile is already
// in M (written before the call; the first barrier below publishes it).
__device__ __forceinline__ bool tile_chol_inv_blk(const double* __restrict__ Akk, int ld,
                                                  double* M, double* Xb, double* Tb, int* okp,
                                                  int nb = 4) {
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  if (Akk != nullptr) {
    // all 16 loads of a lane in flight before the LDS stores
    double tmp[kTB * kTB / kTlWG];
#pragma unroll
    for (int q = 0; q < kTB * kTB / kTlWG; ++q) {
      const int e = t + kTlWG * q;
      tmp[q] = Akk[(size_t)(e >> 6) * ld + (e & 63)];
    }
#pragma unroll
    for (int q = 0; q < kTB * kTB / kTlWG; ++q) {
      const int e = t + kTlWG * q;
      M[(e >> 6) * kMS + (e & 63)] = tmp[q];
    }
  }
  bool ok = true;
  // wave-to-wave hand-offs inside the tile (LDS flags, raised once per call):
  // 0: L_10, 1: L_20, 2: L_30, 3: L_21, 4: L_31, 5: L_32 stored
  // callers pass M = VX, Xb = VX + kTB * kMS, Tb = Xb + 10 * 16 * kBS17 of a
  // VX[2 * kTB * kTB]: M + Xb + Tb + the six flags (3 doubles) must fit in it
  static_assert(kTB * kMS + 13 * 16 * kBS17 + 3 <= 2 * kTB * kTB, "tile factor LDS layout overflows VX");
  int* fl = reinterpret_cast<int*>(Tb + 3 * 16 * kBS17);
  if (t < 6) fl[t] = 0;
  __syncthreads();
  FAC_T(0);
  // One loop over the block columns with ONE instance of wave 0's 16x16 code
  // (an instance per block column measured 0.4-1.0 us slower per block: the
  // unrolled factor is ~16 KB of code and the copies missed the instruction
  // cache).  Wave 0 runs the critical chain with look-ahead: before block p's
  // factor it forms the panel block L_{p,p-1} and the trailing block A_pp
  // itself, so the only workgroup barrier per block column is the one that
  // publishes X_pp.  Waves 1-3 take the other panel and trailing blocks of
  // block column p-1 beside block p's factor (LDS flags for the blocks one
  // wave forms and another reads) and assemble L^-1 block by block as its
  // inputs appear, so that after block 3's factor only X_3p = -X_33 T_3p is
  // left (one 16x16 product per wave):
  //   X_ip = -X_ii T_ip,  T_ip = sum_{k=p}^{i-1} L_ik X_kp  (k ascending).
  // Every block gets the same updates in the same order as the column-by-column
  // form: bit-identical.
  const d4 z = d4{0.0, 0.0, 0.0, 0.0};
  auto T_of = [&](int i, int p, int k_end) {  // sum_{k=p}^{k_end-1} L_ik X_kp
    d4 acc = z;
    for (int k = p; k < k_end; ++k)
      acc = mm16_xy(M + (16 * i) * kMS + 16 * k, kMS, Xb + blk_id(k, p) * 16 * kBS17, kBS17, acc, false);
    return acc;
  };
  auto X_from = [&](int i, int p, d4 T) {  // X_ip = -X_ii T (T through this wave's Tb block)
    double* Tw = Tb + (w - 1) * 16 * kBS17;
    st16(Tw, kBS17, T);
    wave_lds_fence();
    st16(Xb + blk_id(i, p) * 16 * kBS17, kBS17, mm16_xy(Xb + blk_id(i, i) * 16 * kBS17, kBS17, Tw, kBS17, z, true));
    wave_lds_fence();
  };
  auto Mb = [&](int i, int j) { return M + (16 * i) * kMS + 16 * j; };
  auto panel = [&](int i, int p) {  // L_ip = A_ip X_pp^T, in place
    st16(Mb(i, p), kMS, mm16_xyT(Mb(i, p), kMS, Xb + blk_id(p, p) * 16 * kBS17, kBS17, z, false));
    wave_lds_fence();
  };
  auto trail = [&](int i, int j, int p) {  // A_ij -= L_ip L_jp^T
    st16(Mb(i, j), kMS, mm16_xyT(Mb(i, p), kMS, Mb(j, p), kMS, ld16(Mb(i, j), kMS), true));
    wave_lds_fence();
  };
  auto put = [&](int f) {  // this wave's LDS stores before it, then flag f
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    if (l == 0) __hip_atomic_store(fl + f, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  };
  auto get = [&](int f) {
    while (__hip_atomic_load(fl + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0)
      __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  };
  d4 T3 = z;
#pragma unroll 1
  for (int p = 0; p < 4; ++p) {
    if (w == 0) {
      if (SLAM_TL_PADSKIP && p >= nb) {  // a padding block: L_{p,p-1} = 0, L_pp = X_pp = I
        put(p == 1 ? 0 : (p == 2 ? 3 : 5));
        blk_identity_w0(Xb, p);
      } else {
        if (p > 0) {  // look-ahead: L_{p,p-1}, then A_pp's last update
          panel(p, p - 1);
          put(p == 1 ? 0 : (p == 2 ? 3 : 5));
          trail(p, p, p - 1);
        }
        FAC_T(1 + 3 * p);  // (profiling build: block p's look-ahead done)
        blk_factor_w0(M, Xb, p, ok);
      }
    } else if (p == 1) {  // block column 0's other panel and trailing blocks
      if (w == 1) {
        panel(2, 0);
        put(1);
        trail(2, 2, 0);
        get(0);
        trail(2, 1, 0);
      } else if (w == 2) {
        panel(3, 0);
        put(2);
        trail(3, 3, 0);
        get(0);
        trail(3, 1, 0);
      } else {
        get(1);
        get(2);
        trail(3, 2, 0);
      }
    } else if (p == 2) {  // block column 1's, and X_10
      if (w == 1) {
        panel(3, 1);
        put(4);
        trail(3, 3, 1);
      } else if (w == 2) {
        get(3);
        get(4);
        trail(3, 2, 1);
      } else {
        X_from(1, 0, T_of(1, 0, 1));  // X_10 (X_00, X_11: published by the barriers)
      }
    } else if (p == 3) {
      if (w == 1) X_from(2, 1, T_of(2, 1, 2));  // X_21
      if (w == 2) X_from(2, 0, T_of(2, 0, 2));  // X_20 (needs X_10: published by the barrier)
      // wave 1: T_31, wave 2: T_30, wave 3: T_32 (each wave reads only the X
      // blocks it formed itself or that the barrier published), after L_32
      get(5);
      T3 = T_of(3, w == 1 ? 1 : (w == 2 ? 0 : 2), 3);
    }
    if (p < 3) {
      __syncthreads();  // X_pp and block column p-1's blocks published
      FAC_T(3 + 3 * p);
    }
  }
  FAC_T(12);
  __syncthreads();  // X_33 published
  if (w > 0) X_from(3, w == 1 ? 1 : (w == 2 ? 0 : 2), T3);
  if (w == 0 && l == 0) *okp = ok ? 1 : 0;
  __syncthreads();
  FAC_T(13);
  return *okp != 0;
}

// fragment-ordered LDS image of the TRANSPOSE of a 64x64 tile (frag_idx(c, r)
// holds g[r][c]): as the second MFMA operand it gives X Y, as the first Y^T X
__device__ __forceinline__ void tile_to_frag_t(const double* __restrict__ g, int ld, double* f) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, c = lane >> 4;
  for (int f0 = w; f0 < 64; f0 += 16 * (kTlWG / 64)) {
    double tmp[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int fi = f0 + q * (kTlWG / 64);
      tmp[q] = g[(size_t)(4 * (fi & 15) + c) * ld + 16 * (fi >> 4) + r];
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) f[((f0 + q * (kTlWG / 64)) << 6) + lane] = tmp[q];
  }
}

// acc[s] (wave w) += rows 16w.., cols 16s.. of the product of two fragment images
__device__ __forceinline__ void tile_gemm_acc(const double* Xf, const double* Yf, d4 acc[4], bool neg = false) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll 4
  for (int kk = 0; kk < 16; ++kk) {
    const double a0 = Xf[((w * 16 + kk) << 6) + lane];
    const double a = neg ? -a0 : a0;
#pragma unroll
    for (int s = 0; s < 4; ++s)
      acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Yf[((s * 16 + kk) << 6) + lane], acc[s], 0, 0, 0);
  }
}
__device__ __forceinline__ void tile_store(double* C, int ld, const d4 acc[4], bool sub = false) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double* c = C + (size_t)(w * 16 + (lane >> 4) + 4 * r) * ld + s * 16 + (lane & 15);
      *c = sub ? *c - acc[s][r] : acc[s][r];
    }
}

// lower tile (I, J), I >= J, of linear index idx = I (I + 1) / 2 + J
__device__ __forceinline__ int2 lower_tile_of(int idx) {
  int I = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
  while ((I + 1) * (I + 2) / 2 <= idx) ++I;
  while (I * (I + 1) / 2 > idx) --I;
  return int2{I, idx - I * (I + 1) / 2};
}

// ---------------------------------------------------------------- the steps of a tiled solve
// Panel, trailing update and back substitution of a blocked Cholesky over 64x64
// tiles, once for the three solvers (the level-scheduled camera solve, the
// camera covariance, the pose graph's skyline factor).  A solver says where its
// tiles are through a struct with
//   double* at(int I, int J)   first element of lower tile (I, J)
//   ld                         its row stride; its type is the type of a row offset
//                              (size_t in the dense layouts, int in the skyline: with
//                              the other width the compiler waits after every load of
//                              tile_back's row loop, profiles/tile_steps/)
// and passes what only it does as a callable.  Lower tiles (I, J) of a dense
// row-major N x N matrix:
struct DenseTiles {
  double* a;
  size_t ld;
  __device__ __forceinline__ DenseTiles(double* a_, int n) : a(a_), ld((size_t)n) {}
  __device__ __forceinline__ double* at(int I, int J) const { return a + (size_t)I * kTB * ld + J * kTB; }
};

// Panel step of column k by the workgroup of tile (I, k), I >= k; all four
// waves call it.  Every workgroup factors A_kk (L_kk^-1, tile_chol_inv_blk; nb
// as there); the diagonal one (I == k) then runs diag(x, ok, lane, Vf) on wave
// 1 -- x[m] = (L_kk^-1)[m][lane], ok the factor's verdict, Vf 2 * 64 * 64
// doubles of LDS that are the wave's alone -- and the others form L_Ik = A_Ik
// L_kk^-T in place.  *fail != 0: a factor before this one failed, nothing is
// done.  This launch's diagonal workgroup may raise the flag while the others
// start, so one lane reads it for the whole workgroup (a wave that left alone
// would leave the others waiting inside the tile factor).
template <class Tiles, class Diag>
__device__ __forceinline__ void tile_panel(const Tiles& A, int k, int I, int nb, const int* fail, Diag diag) {
  __shared__ double VX[2 * kTB * kTB];
  double* Vf = VX;                        // L_kk^-1, fragment order
  __shared__ double Xf[kTB * kTB];        // A_Ik, fragment order
  __shared__ int okf;
  if (threadIdx.x == 0) okf = *reinterpret_cast<const volatile int*>(fail) != 0 ? 1 : 0;
  __syncthreads();
  if (okf != 0) return;
  __syncthreads();  // okf is written again by the tile factor
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  double* AIk = A.at(I, k);
  if (I > k && w >= 2) tile_to_frag(AIk, (int)A.ld, Xf, w - 2, 2);
  double x[kTB];
  double* Mb = VX;
  double* Xb = VX + kTB * kMS;
  double* Tb = Xb + 10 * 16 * kBS17;
  const bool ok = tile_chol_inv_blk(A.at(k, k), (int)A.ld, Mb, Xb, Tb, &okf, nb);
  if (w == 1) {
    const int cb16 = lane >> 4;
#pragma unroll
    for (int m = 0; m < kTB; ++m)
      x[m] = (m >> 4) >= cb16 ? Xb[blk_id(m >> 4, cb16) * 16 * kBS17 + (m & 15) * kBS17 + (lane & 15)]
                              : 0.0;
  }
  __syncthreads();  // VX is reused below
  if (w == 1) {
    if (I == k) {
      diag(x, ok, lane, Vf);
    } else {
#pragma unroll
      for (int m = 0; m < kTB; ++m) Vf[frag_idx(m, lane)] = x[m];
    }
  }
  if (I == k || !ok) return;
  __syncthreads();
  d4 acc[4];
  gemm_xyT_lowY(Xf, Vf, acc);  // L_Ik = A_Ik (L_kk^-1)^T
  tile_store(AIk, (int)A.ld, acc);
}

// The diagonal workgroup of a solve's panel (tile_panel's diag): L_kk^-1 stored
// row-major into dinv, y_k = L_kk^-1 b_k (row lane's products through LDS,
// summed over rotated columns: no bank conflicts), the flag raised on a failed
// factor.
struct PanelSolveDiag {
  double* dinv;     // L_kk^-1 [64][64]
  const double* b;  // b_k
  double* y;        // y_k
  int* fail;
  __device__ __forceinline__ void operator()(const double (&x)[kTB], bool ok, int lane, double* Vf) const {
    const double bc = b[lane];
#pragma unroll
    for (int m = 0; m < kTB; ++m) dinv[m * kTB + lane] = x[m];
#pragma unroll
    for (int m = 0; m < kTB; ++m) Vf[m * kTB + lane] = x[m] * bc;
    wave_lds_fence();
    double yl = 0.0;
    for (int c = 0; c < kTB; ++c) yl += Vf[lane * kTB + ((c + lane) & 63)];
    y[lane] = yl;
    if (!ok && lane == 0) *fail = 1;
  }
};

// Trailing update of tile (I, J), I >= J, by one workgroup: A_IJ -= sum_k L_Ik
// L_Jk^T over the source columns `cols`, on the f64 matrix cores.  cols is one
// column (an int) or a TileCols list, taken in its order; the one-column form
// has no loop, also not for the compiler (with a loop of one trip k_cov_update
// took 84 registers instead of 78).  RHS: on a diagonal tile also b_I -= sum_k
// L_Ik y_k (y, b: the whole vectors, 64 per tile) -- thread (w, lane) keeps row
// lane's terms [16w, 16w + 16) of every column in one fma chain, the four
// chains summed in wave order.
struct TileCols {
  const int32_t* k;
  int n;
};
template <bool RHS, class Tiles, class Cols>
__device__ __forceinline__ void tile_update(const Tiles& A, int I, int J, Cols cols, const double* y, double* b) {
  __shared__ double Xf[kTB * kTB], Yf[kTB * kTB];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  d4 acc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
  double bs = 0.0;
  auto column = [&](int k) {
    const double* LIk = A.at(I, k);
    tile_to_frag(LIk, (int)A.ld, Xf);
    if (I != J) tile_to_frag(A.at(J, k), (int)A.ld, Yf);
    if constexpr (RHS) {
      if (I == J) {
        const double* yk = y + k * kTB;
        for (int m = 16 * w; m < 16 * w + 16; ++m) bs = __builtin_fma(LIk[lane * A.ld + m], yk[m], bs);
      }
    }
    __syncthreads();
    tile_gemm_acc(Xf, I == J ? Xf : Yf, acc);
  };
  if constexpr (std::is_same_v<Cols, int>) {
    column(cols);
  } else {
    for (int q = 0; q < cols.n; ++q) {
      if (q > 0) __syncthreads();  // Xf / Yf are reloaded
      column(cols.k[q]);
    }
  }
  tile_store(A.at(I, J), (int)A.ld, acc, true);
  if constexpr (RHS) {
    __shared__ double part[4][kTB];
    if (I == J) {
      part[w][lane] = bs;
      __syncthreads();
      if (t < kTB) b[I * kTB + t] -= ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
    }
  }
}

// Back substitution of column k by one workgroup: x_k = L_kk^-T (y_k - sum_u
// L_Ik^T x_I) over the nr row tiles I = row(u), u ascending; dinv: L_kk^-1
// [64][64] row-major, y and x the whole vectors.  Thread (q, c): rows [16q,
// 16q + 16) of every product, column c, in one fma chain; the four chains
// summed in wave order.
template <class Tiles, class Row>
__device__ __forceinline__ void tile_back(const Tiles& A, int k, int nr, Row row, const double* dinv,
                                          const double* y, double* x) {
  __shared__ double r[kTB];
  __shared__ double part[4][kTB];
  const int t = threadIdx.x, c = t & 63, q = t >> 6;
  double s2 = 0.0;
  for (int u = 0; u < nr; ++u) {
    const int I = row(u);
    const double* LIk = A.at(I, k);
    const double* xI = x + I * kTB;
    for (int m = 16 * q; m < 16 * q + 16; ++m) s2 = __builtin_fma(LIk[m * A.ld + c], xI[m], s2);
  }
  part[q][c] = s2;
  __syncthreads();
  if (t < kTB) r[t] = y[k * kTB + t] - (((part[0][t] + part[1][t]) + part[2][t]) + part[3][t]);
  __syncthreads();
  double s3 = 0.0;
  for (int m = 16 * q; m < 16 * q + 16; ++m) s3 = __builtin_fma(dinv[m * kTB + c], r[m], s3);
  part[q][c] = s3;
  __syncthreads();
  if (t < kTB) x[k * kTB + t] = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
}

}  // namespace
