// The tiled camera solve of bundle adjustment (9C > kLdsMaxN): k_tl3_flow, one
// dataflow launch (the default), and k_tl2_*, the same tile operations level by
// level.  ba.hip reaches it through slam::launch_solve_tiled (ba_common.hpp).
// The tile steps themselves (fragment images, tile products, the diagonal-tile
// factor, panel / update / back) are in tile_f64.hpp, shared with the camera
// covariance (ba_cov.hip) and the pose graph (posegraph_se3.hip).
#include "ba_common.hpp"
#include "ba_epilogue.hpp"
#include "tile_f64.hpp"

namespace {

// ---------------------------------------------------------------- tiled solve
// Large reduced camera systems (9C > kLdsMaxN: the sharded C4 window, global
// BA): blocked Cholesky LL^T over 64x64 f64 tiles in the nested-dissection
// tile order of ba.tl_schedule (symbolic structure on the host), two forms:
//   k_tl3_flow    one launch, one persistent workgroup per tile column; device
//                 flags replace launch boundaries (the default);
//   k_tl2_*       the same tile operations level by level as separate launches
//                 (when the columns cannot all be resident: more tiles than
//                 the stream's CUs, or tl_mode "levels").
// Both start from k_tl2_load / k_tl2_scatter (damped S -> lower tiles, b) and
// end in solve_epilogue.  The diagonal-tile factor + inverse is
// tile_chol_inv_blk (16x16 diagonal blocks in wave 0's registers, the rest on
// the f64 matrix cores); it and the fragment / tile-product helpers live in
// tile_f64.hpp, shared with the pose graph's skyline factor.
constexpr int kTlHdr = 12;     // ints of the tile schedule's header
constexpr int kEpiCams = 16;   // cameras per tile in k_tl3_flow's spread epilogue (ba.EPI_CAMS_MAX)

struct TlLayout {  // doubles inside p.chol; T = the schedule's tile count (ba.tl_schedule)
  int T, N;
  long long a, dinv, b, y, x, nz, fail, xo, fc, epi, flow, total;
  __host__ __device__ TlLayout(int n, int n_tiles) {
    T = n_tiles;
    N = T * kTB;
    a = 0;
    dinv = a + (long long)N * N;         // T tiles L_kk^-1 (row-major 64x64 each)
    b = dinv + (long long)N * kTB;
    y = b + N;
    x = y + N;
    nz = x + N;                          // T*T bytes
    fail = nz + ((long long)T * T + 7) / 8;
    xo = fail + 8;                       // fail flag + 7 spare slots (ba.py mirrors this layout)
    fc = xo + N;                         // k_tl3_flow: x in camera order; [T][T][64] L_Ik y_k
    epi = fc + (long long)T * T * kTB;   // (forward-substitution terms); [T][2] epilogue partials
    flow = epi + 2 * T;                  // (pc, cost per tile), then ints: flags
    // tile[T][T], y[T], x[T]; ticket, epoch, start ticket (+5 spare); retired row
    // tiles + waiter mark cnt[T]; L_JJ^-1 / y_J published dv[T]
    total = flow + ((long long)T * T + 4 * T + 8 + 1) / 2;
    // then k_tl3_flow's product slots (tl_sched[11] of them, slam_ba_chol_len):
    // [slots][64][64] terms L_Ik L_Jk^T, then one epoch flag (int) per slot
  }
  __host__ __device__ long long prod(int slot) const { return total + (long long)slot * kTB * kTB; }
  __host__ __device__ long long with_slots(int n_slots) const {
    return prod(n_slots) + ((long long)n_slots + 1) / 2;
  }
};

// Fragment order with the offset inside each 64-double fragment F rotated by
// (4 * (c & 3) + (F & 3)) mod 16 within its 16-row quarter: the MFMA result
// layout (lanes along a row) then stores without LDS bank conflicts (16-way in
// plain fragment order: a 16-lane group's doubles all sit 32 dwords apart),
// and a fragment still reads back conflict-free (a permutation of each quarter).
__device__ __forceinline__ int frag_swz(int r, int c) {
  const int F = ((r >> 4) << 4) + (c >> 2), hi = c & 3;
  return (F << 6) + (hi << 4) + (((r & 15) + 4 * hi + (F & 3)) & 15);
}
// gemm_xyT_lowY with both operands in frag_swz order (same products, same order)
__device__ __forceinline__ void gemm_xyT_lowY_swz(const double* Xf, const double* Yf, d4 acc[4]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int so[4];
#pragma unroll
  for (int k3 = 0; k3 < 4; ++k3) so[k3] = ((lane >> 4) << 4) + (((lane & 15) + 4 * (lane >> 4) + k3) & 15);
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = d4{0.0, 0.0, 0.0, 0.0};
  static_for<0, 16>([&](auto K) {
    constexpr int kk = decltype(K)::value;
    const double a = Xf[((w * 16 + kk) << 6) + so[kk & 3]];
    static_for<kk / 4, 4>([&](auto S) {
      constexpr int s = decltype(S)::value;
      acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Yf[((s * 16 + kk) << 6) + so[kk & 3]], acc[s], 0, 0, 0);
    });
  });
}

__device__ __forceinline__ bool tl_failed(const slam_ba_problem& p, const TlLayout& L) {
  return *reinterpret_cast<const volatile int*>(p.chol + L.fail) != 0;
}

constexpr int kVR = 65;   // row stride of k_tl3_flow's row-major L_JJ^-1

// ---------------------------------------------------------------- level-scheduled tiled solve
// The same tile factor with the columns grouped by elimination-tree level
// (slam355/ba_plan.py tl_schedule: tiles renumbered by nested dissection of the
// tile graph, symbolic structure on the host).  Per level: k_tl2_panel (WG per
// (k, I) of every column k of the level: the diagonal WG stores L_kk^-1 and
// y_k = L_kk^-1 b_k, the others L_Ik = A_Ik L_kk^-T), then k_tl2_update (WG
// per target tile (I, J) of the level: A_IJ -= sum_k L_Ik L_Jk^T on the f64
// matrix cores, and for I = J also b_I -= sum_k L_Ik y_k -- the sums over the
// level's columns inside one WG, no atomics).  k_tl2_back walks the levels in
// reverse: x_k = L_kk^-T (y_k - sum_I L_Ik^T x_I) over the ancestors I; then
// k_tl2_unperm moves x back to the camera order (into the y region, which the
// epilogue reads).  A banded window of T tiles runs ~log2 T levels instead of
// T panel steps (C4: 4 levels for 9 tiles; C5: 8 for 71).
// The schedule's row maps sit at fixed offsets after its kTlHdr-int header (ba.tl_schedule;
// checked on the host in tl_check_sched), so no lookup waits on a header load:
// row r of S (camera order) -> its row in the tiled system
__device__ __forceinline__ int tl_new_row(const int32_t* sched, int r) { return sched[kTlHdr + r]; }
// row of the tiled system -> row of S, -1 on a tile's padding rows
__device__ __forceinline__ int tl_old_row(const int32_t* sched, int n, int rn) { return sched[kTlHdr + n + rn]; }
// rows of S in tile k (they come first, padding after them)
__device__ __forceinline__ const int32_t* tl_tile_rows(const int32_t* sched, int n, int T) {
  return sched + kTlHdr + n + T * kTB;
}

// Zero the lower tiles (identity on the padded rows' diagonal), b in the new order.
// struct_only: only the tiles the symbolic factor touches -- (J, J) and (I, J)
// for the rows I of column J (column table; grid T x (1 + max rows)); every
// other lower tile is never read by either solve form (C5: 71 diagonal + row
// tiles of 2556 lower tiles).  Otherwise all T (T + 1) / 2 lower tiles.
__global__ __launch_bounds__(kTlWG) void k_tl2_load(slam_ba_problem p, int T_, int struct_only) {
  lm_wave_priority();
  const int n = 9 * p.n_cams;
  const TlLayout L(n, T_);
  const int32_t* S = p.tl_sched;
  int I, J;
  bool first;
  if (struct_only) {
    J = blockIdx.x;
    const int q = blockIdx.y;
    const int32_t* rec = S + S[5] + 5 * J;
    if (q > rec[1]) return;  // uniform; (0, 0) always runs
    I = q == 0 ? J : S[rec[0] + q - 1];
    first = blockIdx.x == 0 && q == 0;
  } else {
    const int2 IJ = lower_tile_of(blockIdx.x);
    I = IJ.x;
    J = IJ.y;
    first = blockIdx.x == 0;
  }
  double* A = p.chol + L.a;
  for (int e = threadIdx.x; e < kTB * kTB; e += kTlWG) {
    const int i = I * kTB + (e >> 6), j = J * kTB + (e & 63);
    A[(size_t)i * L.N + j] = (i == j && tl_old_row(S, n, i) < 0) ? 1.0 : 0.0;  // identity on padding
  }
  if (I == J && threadIdx.x < kTB) {
    const int r = tl_old_row(S, n, I * kTB + threadIdx.x);  // row of S landing at new row I*64 + t
    p.chol[L.b + I * kTB + threadIdx.x] = r >= 0 ? p.sys[sys_vec_off(p.n_cams, p.n_blocks) + r] : 0.0;
  }
  if (first) {
    // k_tl3_flow: a new solve epoch (its flags compare against it); the retire
    // ticket, the start ticket and the per-column parent counters re-armed
    int* fl = reinterpret_cast<int*>(p.chol + L.flow) + L.T * L.T + 2 * L.T;
    for (int i = threadIdx.x; i < L.T; i += blockDim.x) fl[8 + i] = 0;
    if (threadIdx.x == 0) {
      *reinterpret_cast<int*>(p.chol + L.fail) = 0;
      fl[0] = 0;
      fl[1] = fl[1] + 1;
      fl[2] = 0;
    }
  }
}

// One WG per packed block: its values at their renumbered positions (lower
// tiles, full symmetric inside diagonal tiles), camera damping on the diagonal.
__global__ __launch_bounds__(128) void k_tl2_scatter(slam_ba_problem p, int T_) {
  lm_wave_priority();
  const int n = 9 * p.n_cams;
  const TlLayout L(n, T_);
  const int32_t* S = p.tl_sched;
  const int blk = blockIdx.x, t = threadIdx.x;
  if (t >= 81) return;
  const int c1 = p.blocks[2 * blk], c2 = p.blocks[2 * blk + 1];
  const double* vec = p.sys + sys_vec_off(p.n_cams, p.n_blocks);
  const int i = t / 9, j = t - 9 * (t / 9);
  const int r = 9 * c1 + i, c = 9 * c2 + j;  // element (r, c) of S
  double v = p.sys[(size_t)blk * 81 + t];
  if (r == c) v += p.state[SLAM_BA_ST_LAMBDA] * clampd(vec[2 * n + r]);
  double* A = p.chol + L.a;
  const int rn = tl_new_row(S, r), cn = tl_new_row(S, c);
  const int tr = rn / kTB, tc = cn / kTB;
  if (tr >= tc) A[(size_t)rn * L.N + cn] = v;
  if (c1 != c2 && tc >= tr) A[(size_t)cn * L.N + rn] = v;
}

__global__ __launch_bounds__(kTlWG) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_tl2_panel(slam_ba_problem p, int T_, int eoff) {
  lm_wave_priority();
  const TlLayout L(9 * p.n_cams, T_);
  const int32_t* S = p.tl_sched;
  const int k = S[eoff + 2 * blockIdx.x], I = S[eoff + 2 * blockIdx.x + 1];
  int* fail = reinterpret_cast<int*>(p.chol + L.fail);
  tile_panel(DenseTiles(p.chol + L.a, L.N), k, I, (tl_tile_rows(S, 9 * p.n_cams, T_)[k] + 15) >> 4, fail,
             PanelSolveDiag{p.chol + L.dinv + (size_t)k * kTB * kTB, p.chol + L.b + k * kTB,
                            p.chol + L.y + k * kTB, fail});
}

__global__ __launch_bounds__(kTlWG) void k_tl2_update(slam_ba_problem p, int T_, int eoff) {
  lm_wave_priority();
  const TlLayout L(9 * p.n_cams, T_);
  if (tl_failed(p, L)) return;
  const int32_t* S = p.tl_sched;
  const int32_t* e = S + eoff + 4 * blockIdx.x;
  const int I = e[0], J = e[1], ko = e[2], kc = e[3];  // the level's columns k = S[ko .. ko + kc) that reach (I, J)
  tile_update<true>(DenseTiles(p.chol + L.a, L.N), I, J, TileCols{S + ko, kc}, p.chol + L.y, p.chol + L.b);
}

// x_k = L_kk^-T (y_k - sum_I L_Ik^T x_I), I over the column's structure (ancestors).
__global__ __launch_bounds__(kTlWG) void k_tl2_back(slam_ba_problem p, int T_, int eoff) {
  lm_wave_priority();
  const TlLayout L(9 * p.n_cams, T_);
  if (tl_failed(p, L)) return;
  const int32_t* S = p.tl_sched;
  const int32_t* e = S + eoff + 3 * blockIdx.x;
  const int k = e[0], so = e[1], sc = e[2];
  tile_back(DenseTiles(p.chol + L.a, L.N), k, sc, [&](int u) { return S[so + u]; },
            p.chol + L.dinv + (size_t)k * kTB * kTB, p.chol + L.y, p.chol + L.x);
}

// x (new tile order, L.x) -> camera order in the y region (read by the epilogue)
__global__ __launch_bounds__(kTB) void k_tl2_unperm(slam_ba_problem p, int T_) {
  const TlLayout L(9 * p.n_cams, T_);
  const int I = blockIdx.x;  // new tile
  const int r = tl_old_row(p.tl_sched, 9 * p.n_cams, I * kTB + threadIdx.x);
  if (r >= 0) p.chol[L.y + r] = p.chol[L.x + I * kTB + threadIdx.x];
}

__global__ __launch_bounds__(1024) void k_tl2_epilogue(slam_ba_problem p, int T_) {
  lm_wave_priority();
  __shared__ double red[32];
  const int n = 9 * p.n_cams;
  const TlLayout L(n, T_);
  const bool ok = !tl_failed(p, L);
  const double* bvec = p.sys + sys_vec_off(p.n_cams, p.n_blocks);
  const double* gvec = bvec + n;
  solve_epilogue<true>(p, p.chol + L.y, ok, red,
                       EpiSrc{gvec, bvec + 2 * n, p.cams[cur_of(p.state)], gvec + 2 * n});
}

// ---------------------------------------------------------------- dataflow tiled solve
// The same factor as a dataflow graph in ONE launch: workgroup J owns tile
// column J (new numbering) for the whole solve and, from the schedule's column
// table (slam355/ba_plan.py tl_schedule),
//   (1) A_JJ -= sum_{k in rs(J)} L_Jk L_Jk^T  (waits for each L_Jk's flag),
//       factor + inverse of the diagonal tile (tile_chol_inv_blk, from LDS);
//   (2) per row tile I in rows(J), parent first: A_IJ -= sum_k L_Ik L_Jk^T,
//       L_IJ = A_IJ L_JJ^-T, published (tile flag);
//   (3) y_J = L_JJ^-1 (b_J - sum_{k in rs(J)} L_Jk y_k)  (waits for y_k);
//   (4) x_J = L_JJ^-T (y_J - sum_{I in rows(J)} L_IJ^T x_I)  (waits for x_I),
//       stored in the new order and in camera order;
//   (5) the last column to finish (ticket) runs the solve epilogue.
// Launch boundaries become device flags: a column starts as soon as the tiles
// it needs exist, so the factor advances along the elimination tree with no
// per-level launch gaps.  Data crossing workgroups (L tiles, L_JJ^-1, y, x) is
// written with sc1 (write-through) stores and read with sc1 loads; a flag is
// raised after the writer's stores have drained (s_waitcnt + barrier) and
// equals the solve's epoch (bumped by k_tl2_load), so flags never need clearing.
// No residency assumption: a workgroup takes its column from a start
// ticket, so the columns are handed out in the order the workgroups actually
// start, and steps (1)-(3) wait only on lower columns -- workgroups that have
// already started and cannot be descheduled.  The back substitution (4) never
// waits on a later column: x_J is computed by the workgroup that retires the
// LAST of J's row tiles' x (a per-column counter; the roots by their own
// workgroup), so a column whose workgroup finished its forward part long ago,
// or a workgroup that has not started yet, holds nothing up.  The solve is
// therefore correct with any number of its workgroups resident (a CU-masked
// stream, other streams' kernels holding the CUs), and bit-identical whichever
// workgroup computes a column.  Every wait still gives up when the solve failed
// (non-SPD tile) or after kFlowSpinMax polls (a safety net that then marks the
// solve failed: SOLVE_FAULT), and every column is retired exactly once, so the
// retire ticket always reaches T and its last adder runs the epilogue.
constexpr int kFlowSpinMax = 1 << 22;  // ~0.2 s of 128-cycle polls
#ifndef SLAM_FLOW_SLEEP
#define SLAM_FLOW_SLEEP 2  // s_sleep between flag polls (units of 64 clocks)
#endif

#ifdef SLAM_FLOW_PROFILE
// per column: wall clock (100 MHz) at start, diagonal updates done, factor done,
// row tiles published, y published, x inputs in, x published, end
__device__ unsigned long long g_flow_stamp[SLAM_TL_FLOW_MAX_T][8];
// (stamps are kept per COLUMN: the workgroup's own column J, and (5), (6) for
// the column k whose x it formed)
#define FLOW_TC(col, i)                                           \
  do {                                                            \
    if (threadIdx.x == 0) g_flow_stamp[(col)][i] = wall_clock64(); \
  } while (0)
// finer stamps of the same column: first child tile in, last child tile in,
// row 0's deferred folds done, row 0 staged, row 0's product done, row 0 published
__device__ unsigned long long g_flow_sub[SLAM_TL_FLOW_MAX_T][8];
// The own column's stamps go to LDS (flow_lds: 0-4 phases, 8-13 sub-stamps)
// and out to global memory at the end, so that no stamp store is pending at
// the phases' own s_waitcnt vmcnt(0).
#define FLOW_LDS(i)                                               \
  do {                                                            \
    if (threadIdx.x == 0) flow_lds[i] = wall_clock64();           \
  } while (0)
#define FLOW_S(i) FLOW_LDS(8 + (i))
#define FLOW_T(i) FLOW_LDS(i)
#define FLOW_FLUSH()                                                             \
  do {                                                                           \
    if (threadIdx.x == 0) {                                                      \
      for (int i_ = 0; i_ < 5; ++i_) g_flow_stamp[J][i_] = flow_lds[i_];         \
      for (int i_ = 0; i_ < 6; ++i_) g_flow_sub[J][i_] = flow_lds[8 + i_];       \
      g_flow_sub[J][6] = flow_lds[5];                                            \
      g_flow_sub[J][7] = flow_lds[6];                                            \
    }                                                                            \
  } while (0)
#else
#define FLOW_TC(col, i) (void)0
#define FLOW_S(i) (void)0
#define FLOW_T(i) (void)0
#define FLOW_FLUSH() (void)0
#endif

struct FlowPtrs {
  int *tile, *yf, *xf, *ticket, *epoch, *start, *fail, *cnt, *dv, *pf;
  __device__ FlowPtrs(const slam_ba_problem& p, const TlLayout& L) {
    int* base = reinterpret_cast<int*>(p.chol + L.flow);
    tile = base;
    yf = base + L.T * L.T;
    xf = yf + L.T;
    ticket = xf + L.T;
    epoch = ticket + 1;
    start = ticket + 2;
    fail = ticket + 3;  // k_tl3_flow's epoch-tagged fail word
    cnt = ticket + 8;
    dv = cnt + L.T;
    pf = reinterpret_cast<int*>(p.chol + L.prod(p.tl_sched[11]));  // product slot flags
  }
};

__device__ __forceinline__ int ld_flag(const int* f) {
  return __hip_atomic_load(const_cast<int*>(f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_flag(int* f, int v) {
  __hip_atomic_store(f, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The dataflow solve's fail word carries its solve: (epoch << 2) | code, code
// 1 a non-SPD tile, 2 a timed-out wait -- so no launch has to clear it
__device__ __forceinline__ int flow_fcode(const int* fail, int epoch) {
  const int v = ld_flag(fail);
  return (v >> 2) == epoch ? (v & 3) : 0;
}
__device__ __forceinline__ void flow_fail(int* fail, int epoch, int code) { st_flag(fail, (epoch << 2) | code); }

// Thread 0 polls until up() holds; false (uniform) when the solve failed or
// the wait timed out (which marks it failed).
template <typename Up>
__device__ __forceinline__ bool flow_poll(Up up, int epoch, int* fail, int* sh) {
  if (threadIdx.x == 0) {
    int ok = 1;
    for (int spins = 0; !up(); ++spins) {
      if (flow_fcode(fail, epoch) != 0) {
        ok = 0;
        break;
      }
      if (spins > kFlowSpinMax) {
        flow_fail(fail, epoch, 2);
        ok = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(SLAM_FLOW_SLEEP);
    }
    *sh = ok;
  }
  __syncthreads();
  const bool ok = *sh != 0;
  __syncthreads();
  return ok;
}
// ... until *flag == epoch
__device__ bool flow_wait(const int* flag, int epoch, int* fail, int* sh) {
  return flow_poll([=] { return ld_flag(flag) == epoch; }, epoch, fail, sh);
}
// ... until the low half (retired row tiles) of column J's parent counter
// reaches rc -- the retirers' x stores drained before their adds (the counter
// is the acquire for those bytes)
__device__ bool flow_wait_count(const int* cnt, int rc, int epoch, int* fail, int* sh) {
  return flow_poll([=] { return (ld_flag(cnt) & 0xffff) >= rc; }, epoch, fail, sh);
}

// Wave 0 polls base[idx[i]] == epoch for all i < cnt together (lane i, chunks
// of 64), so flags that are already up cost one round trip, not cnt.
__device__ bool flow_wait_many(const int* base, const int32_t* idx, int cnt, int epoch, int* fail,
                               int* sh) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    int ok = 1;
    for (int c0 = 0; c0 < cnt && ok; c0 += 64) {
      const int* f = c0 + lane < cnt ? base + idx[c0 + lane] : nullptr;
      for (int spins = 0;; ++spins) {
        const bool up = f == nullptr || ld_flag(f) == epoch;
        if (__all(up)) break;
        if (flow_fcode(fail, epoch) != 0) {
          ok = 0;
          break;
        }
        if (spins > kFlowSpinMax) {
          if (lane == 0) flow_fail(fail, epoch, 2);
          ok = 0;
          break;
        }
        __builtin_amdgcn_s_sleep(SLAM_FLOW_SLEEP);
      }
    }
    if (lane == 0) *sh = ok;
  }
  __syncthreads();
  const bool ok = *sh != 0;
  __syncthreads();
  return ok;
}

// every thread's (sc1) stores drained, then thread 0 raises the flag
__device__ __forceinline__ void flow_publish(int* flag, int epoch) {
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) st_flag(flag, epoch);
}

// tile_to_frag through sc1 loads (the tile was written by another workgroup)
__device__ __forceinline__ void tile_to_frag_sc1(const double* __restrict__ g, int ld, double* f) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, c = lane >> 4;
  double tmp[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int fi = w + 4 * q;
    tmp[q] = ld_sc1(g + (size_t)(16 * (fi >> 4) + r) * ld + 4 * (fi & 15) + c);
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) f[((w + 4 * q) << 6) + lane] = tmp[q];
}

// two tiles through sc1 loads, all 32 loads of a lane in flight before the LDS stores
__device__ __forceinline__ void tiles2_to_frag_sc1(const double* __restrict__ g0, const double* __restrict__ g1,
                                                   int ld, double* f0, double* f1) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, c = lane >> 4;
  double t0[16], t1[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int fi = w + 4 * q;
    const size_t o = (size_t)(16 * (fi >> 4) + r) * ld + 4 * (fi & 15) + c;
    t0[q] = ld_sc1(g0 + o);
    t1[q] = ld_sc1(g1 + o);
  }
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    f0[((w + 4 * q) << 6) + lane] = t0[q];
    f1[((w + 4 * q) << 6) + lane] = t1[q];
  }
}

// Elements of the damped tiled system gathered straight from the packed S
// (what k_tl2_load + k_tl2_scatter lay out for the level-scheduled solve),
// through the schedule's per-column gather tables (ba.tl_schedule): gt = the
// tile's [64][64] packed-S offsets (-1 zero, -2 a padding row's unit
// diagonal).  Two rounds of independent loads for all N elements (offsets,
// then values); dg: the diagonal tile's rows of S, for lambda clamp(diag U) on
// its diagonal (null for a row tile).
template <int N>
__device__ __forceinline__ void tl_gather(const double* __restrict__ sys, const int32_t* gt,
                                          const int32_t* dg, const double* dU, double lam,
                                          const int (&ri)[N], const int (&ci)[N], double* out) {
  int g[N], r[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    g[i] = gt[ri[i] * kTB + ci[i]];
    r[i] = dg != nullptr && ri[i] == ci[i] ? dg[ri[i]] : -1;
  }
  double v[N], d[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    v[i] = sys[max(g[i], 0)];
    d[i] = r[i] >= 0 ? dU[r[i]] : 0.0;
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double x = g[i] >= 0 ? v[i] : (g[i] == -2 ? 1.0 : 0.0);
    if (r[i] >= 0) x += lam * clampd(d[i]);
    out[i] = x;
  }
}

// lower 16x16 blocks (row, column) of the diagonal update per wave of k_tl3_flow
__constant__ int kDiagBlk[4][3][2] = {{{0, 0}, {3, 0}, {3, 1}}, {{1, 0}, {1, 1}, {3, 2}},
                                      {{2, 0}, {2, 1}, {2, 0}}, {{2, 2}, {3, 3}, {2, 2}}};

__global__ __launch_bounds__(kTlWG) __attribute__((amdgpu_waves_per_eu(1, 1)))
void k_tl3_flow(slam_ba_problem p, int T_) {
  lm_wave_priority();
  const int n = 9 * p.n_cams;
  const TlLayout L(n, T_);
  const int32_t* S = p.tl_sched;
  const int T = L.T;
  const FlowPtrs F(p, L);
  __shared__ double VX[2 * kTB * kTB];  // factor scratch; then L_JJ^-1 (fragments) | operand Y
  __shared__ double Xf[kTB * kTB];      // operand X
  __shared__ double part[4][kTB];
  __shared__ double yv[kTB];
  __shared__ double rv[kTB];
  __shared__ int shf, okf, col_sh, ep_sh;
  __shared__ double VR[kTB * kVR];        // L_JJ^-1 row-major (stride 65): (3), this column's x
  __shared__ int stk[SLAM_TL_FLOW_MAX_T], sp_sh, cur_sh, last_sh, own_sh;
#ifdef SLAM_FLOW_PROFILE
  __shared__ unsigned long long flow_lds[16];
#endif
  // the column: the start ticket hands them out in the order the workgroups
  // start.  The ticket is never reset: every solve takes exactly T tickets, so
  // ticket v is column v mod T of solve v / T, whose number is the epoch that
  // every flag of this solve carries (no clearing launch before the solve)
  if (threadIdx.x == 0) {
    const unsigned v = ticket_add(reinterpret_cast<uint32_t*>(F.start));
    col_sh = (int)(v % (unsigned)T);
    ep_sh = (int)(v / (unsigned)T) + 1;
  }
  __syncthreads();
  const int J = col_sh;
  const int epoch = ep_sh;
  const int32_t* rec = S + S[5] + 5 * J;
  const int ro = rec[0], rc = rec[1], so = rec[2], sc = rec[3], uo = rec[4];
  // rows of the tile (its rows of S first, padding after them): the 16-row
  // blocks of the factor
  const int nbJ = (tl_tile_rows(S, n, T)[J] + 15) >> 4;
  // Product tasks (ba.tl_schedule): the terms L_Ik L_Jk^T of a column J's rows
  // 0 and 1 are formed by column k itself, as soon as both of its tiles exist,
  // into slots that J sums after its factor -- J's diagonal phase never waits
  // for a child's later row tiles, which its children publish after the L_Jk
  // that phase needs.  This column's tasks (a, b, slot), ordered by b.
  const int32_t* tkJ = S + S[S[10] + 2 * J];
  const int n_tk = S[S[10] + 2 * J + 1];
  double* prod = p.chol + L.prod(0);
  // (4b)'s inputs for the cameras this column owns, loaded before any wait:
  // thread t < 9 e_cnt takes row t % 9 of owned camera t / 9
  const double* bvec = p.sys + sys_vec_off(p.n_cams, p.n_blocks);  // b | g | diag U | cost
  const int cur = cur_of(p.state);
  const double lam = p.state[SLAM_BA_ST_LAMBDA];
  const int32_t* erJ = S + S[7] + 2 * J;
  const int e_off = erJ[0], e_cnt = erJ[1];
  int e_row = 0, e_rn = 0;
  double e_cam = 0.0, e_du = 0.0, e_g = 0.0, e_cost = 0.0;
  if (threadIdx.x < 9 * e_cnt) {
    e_row = 9 * S[e_off + threadIdx.x / 9] + threadIdx.x % 9;
    e_rn = tl_new_row(S, e_row);
    e_cam = p.cams[cur][e_row];
    e_g = bvec[n + e_row];
    e_du = bvec[2 * n + e_row];
  }
  if (threadIdx.x < e_cnt) e_cost = bvec[3 * n + S[e_off + threadIdx.x]];
  const int own_orow = threadIdx.x < kTB ? tl_old_row(S, n, J * kTB + threadIdx.x) : -1;
  const double b_own = own_orow >= 0 ? bvec[own_orow] : 0.0;  // b_J in the tiled order (3)
  int* fail = F.fail;
  // this column's parent counter, re-armed before any tile of J is published:
  // no row tile of J can retire before J's tiles exist (x_I needs L_IJ)
  if (threadIdx.x == 0) st_flag(F.cnt + J, 0);
  // this column's gather tables: its diagonal tile, row tile q at 1 + q, the
  // diagonal tile's rows of S after them
  const int32_t* gtJ = S + S[S[9] + J];
  const int32_t* dgJ = gtJ + (1 + rc) * kTB * kTB;
  const double* dU = bvec + 2 * n;
  double* A = p.chol + L.a;
  double* Vf = VX;
  double* Yf = VX + kTB * kTB;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  bool ok = true;
  FLOW_T(0);
  // The diagonal update is symmetric and the factor reads only lower blocks:
  // the 10 lower 16x16 blocks, three per wave (waves 2 and 3 repeat one block
  // they do not store), so each SIMD's MFMA chain per child tile is 48 steps
  // instead of 64.
  int dR[3], dC[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    dR[b] = kDiagBlk[w][b][0];
    dC[b] = kDiagBlk[w][b][1];
  }
  const int dnb = w < 2 ? 3 : 2;
  // A_JJ's blocks, gathered from the packed system into registers before any
  // wait (no load / scatter launch before the solve)
  double ajj[12];
  {
    int gi[12], gj[12];
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        gi[4 * b + r] = dR[b] * 16 + (lane >> 4) + 4 * r;
        gj[4 * b + r] = dC[b] * 16 + (lane & 15);
      }
    tl_gather<12>(p.sys, gtJ, dgJ, dU, lam, gi, gj, ajj);
  }
  // ... and the first two row tiles' A_IJ
  double air[2][16];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    int gi[16], gj[16];
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        gi[4 * s2 + r] = w * 16 + (lane >> 4) + 4 * r;
        gj[4 * s2 + r] = s2 * 16 + (lane & 15);
      }
    tl_gather<16>(p.sys, gtJ + (q < rc ? 1 + q : 0) * kTB * kTB, nullptr, dU, lam, gi, gj, air[q]);
  }
  // (1) diagonal tile, child tiles k in rs order: L_Jk operands double-buffered
  // (Xf / VX[4096:]); the next child's tile is fetched before this one's MFMAs
  // when its flag is already up (loads in flight under the MFMAs), after them
  // otherwise (a child that is not ready yet never holds up the MFMAs of the
  // ones that are).  Row tiles 0 and 1 take their updates from the product
  // slots after the factor (2).
  d4 acc[4];
#pragma unroll
  for (int s2 = 0; s2 < 4; ++s2) acc[s2] = d4{0.0, 0.0, 0.0, 0.0};
  // The buffers alternate so that the LAST child's L_Jk lands in Xf.
  if (sc > 0) {
    ok = flow_wait(F.tile + J * T + S[so], epoch, fail, &shf);
    if (ok) tile_to_frag_sc1(A + (size_t)J * kTB * L.N + S[so] * kTB, L.N, ((sc - 1) & 1) ? Yf : Xf);
    FLOW_S(0);
  }
  for (int q = 0; q < sc && ok; ++q) {
    double* cur = ((sc - 1 - q) & 1) ? Yf : Xf;
    double* nxt = ((sc - 1 - q) & 1) ? Xf : Yf;
    __syncthreads();  // cur filled; the previous MFMAs' reads of nxt done
    if (q == sc - 1) FLOW_S(1);
    bool pre = false;
    if (q + 1 < sc) {
      if (t == 0) shf = ld_flag(F.tile + J * T + S[so + q + 1]) == epoch ? 1 : 0;
      __syncthreads();
      pre = shf != 0;
      __syncthreads();
      if (pre) tile_to_frag_sc1(A + (size_t)J * kTB * L.N + S[so + q + 1] * kTB, L.N, nxt);
    }
#pragma unroll 4
    for (int kk = 0; kk < 16; ++kk)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[((dR[b] * 16 + kk) << 6) + lane],
                                                      cur[((dC[b] * 16 + kk) << 6) + lane], acc[b], 0, 0, 0);
    if (q + 1 < sc) {
      if (!pre) {
        ok = flow_wait(F.tile + J * T + S[so + q + 1], epoch, fail, &shf);
        if (ok) tile_to_frag_sc1(A + (size_t)J * kTB * L.N + S[so + q + 1] * kTB, L.N, nxt);
      }
    }
  }
  __syncthreads();
  FLOW_T(1);
  if (ok) {
    double* M = VX;  // lower blocks only (tile_chol_inv_blk reads no others)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      if (b < dnb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = dR[b] * 16 + (lane >> 4) + 4 * r, col = dC[b] * 16 + (lane & 15);
          M[row * kMS + col] = ajj[4 * b + r] - acc[b][r];
        }
      }
    double* Xb = VX + kTB * kMS;
    ok = tile_chol_inv_blk(nullptr, 0, M, Xb, Xb + 10 * 16 * kBS17, &okf, nbJ);
    // L_JJ^-1 out of the block store into (swizzled) fragment order (Vf) and
    // row-major (VR): wave w takes rows [16w, 16w + 16), lane = column
    double x[16];
    if (ok) {
      const int cb16 = lane >> 4;
#pragma unroll
      for (int m = 0; m < 16; ++m)
        x[m] = w >= cb16 ? Xb[blk_id(w, cb16) * 16 * kBS17 + m * kBS17 + (lane & 15)] : 0.0;
    }
    __syncthreads();  // VX is reused below
    if (!ok) {
      if (t == 0) flow_fail(fail, epoch, 1);
    } else {
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        Vf[frag_swz(16 * w + m, lane)] = x[m];
        VR[(16 * w + m) * kVR + lane] = x[m];
      }
    }
    __syncthreads();
  }
  FLOW_T(2);
  // (2) row tiles, parent first.  Rows 0 and 1 (the children folded in during
  // (1), A_IJ in registers) and the rest are separate straight-line instances:
  // one uniform branch per row tile, not one per element (this code runs once
  // per solve on a CU whose instruction cache the LM kernels have refilled, so
  // every taken branch into cold code costs an L2 fetch).
  double l0[16];  // L_{rows[0]} J, kept for this column's product tasks with a = 0
  auto row_tile = [&](auto QC, int q) {
    constexpr int qc = decltype(QC)::value;  // 0, 1: rows 0 / 1; 2: any later row
    const int I = S[ro + q];
    const int ko = S[uo + 2 * q], kc = S[uo + 2 * q + 1];
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) acc[s2] = d4{0.0, 0.0, 0.0, 0.0};
    // Rows 0 and 1: the k list's product slots (after the list), summed in list
    // order, each a 64x64 term in the accumulator layout; the staged A_IJ goes
    // to Yf.  Later rows load both tiles (loads in flight together), MFMA the
    // term here and stage into Xf.
    double* stg = qc < 2 ? Yf : Xf;
    if constexpr (qc < 2) {
      if (kc > 0) ok = flow_wait_many(F.pf, S + ko + kc, kc, epoch, fail, &shf);
#ifdef SLAM_FLOW_PROFILE
      if (q == 0) FLOW_LDS(5);
#endif
      for (int u0 = 0; u0 < kc && ok; u0 += 2) {
        double cv[2][16];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const double* Cp = prod + (size_t)S[ko + kc + min(u0 + h, kc - 1)] * kTB * kTB;
#pragma unroll
          for (int e = 0; e < 16; ++e) cv[h][e] = ld_sc1(Cp + ((4 * w + (e >> 2)) * 4 + (e & 3)) * 64 + lane);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
          if (u0 + h < kc) {
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[s2][r] += cv[h][4 * s2 + r];
          }
      }
#ifdef SLAM_FLOW_PROFILE
      if (q == 0) FLOW_LDS(6);
#endif
    } else {
      for (int u = 0; u < kc && ok; ++u) {
        const int k = S[ko + u];
        ok = flow_wait(F.tile + I * T + k, epoch, fail, &shf);  // (J, k) was waited for in (1)
        if (!ok) break;
        tiles2_to_frag_sc1(A + (size_t)I * kTB * L.N + k * kTB, A + (size_t)J * kTB * L.N + k * kTB, L.N,
                           Yf, Xf);
        __syncthreads();
        tile_gemm_acc(Yf, Xf, acc);
        __syncthreads();
      }
    }
    if (!ok) return;
    if (q == 0) FLOW_S(2);
    double* AIJ = A + (size_t)I * kTB * L.N + J * kTB;
    double a[16];
    if constexpr (qc < 2) {
#pragma unroll
      for (int e = 0; e < 16; ++e) a[e] = air[qc][e];
    } else {
      int gi[16], gj[16];
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          gi[4 * s2 + r] = w * 16 + (lane >> 4) + 4 * r;
          gj[4 * s2 + r] = s2 * 16 + (lane & 15);
        }
      tl_gather<16>(p.sys, gtJ + (1 + q) * kTB * kTB, nullptr, dU, lam, gi, gj, a);
    }
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = w * 16 + (lane >> 4) + 4 * r, col = s2 * 16 + (lane & 15);
        stg[frag_swz(row, col)] = a[4 * s2 + r] - acc[s2][r];
      }
    __syncthreads();
    if (q == 0) FLOW_S(3);
    d4 lacc[4];
    gemm_xyT_lowY_swz(stg, Vf, lacc);  // L_IJ = A_IJ (L_JJ^-1)^T
#ifdef SLAM_FLOW_PROFILE
    if (q == 0) {
      __builtin_amdgcn_s_waitcnt(0);
      FLOW_S(4);
    }
#endif
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = w * 16 + (lane >> 4) + 4 * r, col = s2 * 16 + (lane & 15);
        st_sc1(AIJ + (size_t)row * L.N + col, lacc[s2][r]);
      }
    flow_publish(F.tile + I * T + J, epoch);
    if (q == 0) FLOW_S(5);
    if (q == 0) {
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
        for (int r = 0; r < 4; ++r) l0[4 * s2 + r] = lacc[s2][r];
    }
    // this column's product tasks with b = q: L_IJ (this row tile, X operand)
    // times L_{rows[a]} J^T (row 0 from registers, others reloaded), into the
    // slot; the publish's barrier ended every read of Xf / Yf
    bool xs = false;
    for (int e = 0; e < n_tk; ++e) {
      if (tkJ[3 * e + 1] != q) continue;  // (uniform)
      const int ta = tkJ[3 * e], slot = tkJ[3 * e + 2];
      if (!xs) {
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            Xf[frag_idx(w * 16 + (lane >> 4) + 4 * r, s2 * 16 + (lane & 15))] = lacc[s2][r];
        xs = true;
      }
      if (ta == 0) {
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            Yf[frag_idx(w * 16 + (lane >> 4) + 4 * r, s2 * 16 + (lane & 15))] = l0[4 * s2 + r];
      } else {
        tile_to_frag_sc1(A + (size_t)S[ro + ta] * kTB * L.N + J * kTB, L.N, Yf);
      }
      __syncthreads();
      d4 pacc[4];
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2) pacc[s2] = d4{0.0, 0.0, 0.0, 0.0};
      tile_gemm_acc(Xf, Yf, pacc);
      double* Cp = prod + (size_t)slot * kTB * kTB;
#pragma unroll
      for (int s2 = 0; s2 < 4; ++s2)
#pragma unroll
        for (int r = 0; r < 4; ++r) st_sc1(Cp + ((4 * w + s2) * 4 + r) * 64 + lane, pacc[s2][r]);
      flow_publish(F.pf + slot, epoch);  // (its barrier also ends this task's Yf reads)
    }
  };
  if (ok && rc > 0) row_tile(std::integral_constant<int, 0>{}, 0);
  if (ok && rc > 1) row_tile(std::integral_constant<int, 1>{}, 1);
  for (int q = 2; q < rc && ok; ++q) row_tile(std::integral_constant<int, 2>{}, q);
  FLOW_T(3);
  // (3) forward substitution: r = b_J - sum_{k in rs(J)} L_Jk y_k, the terms
  // pushed by the children (fc[J][k]); y_J = L_JJ^-1 r; then this column's
  // own terms L_IJ y_J for its rows I (fc[I][J]), published with the y flag
  if (ok) ok = flow_wait_many(F.yf, S + so, sc, epoch, fail, &shf);
  if (ok) {
    if (t < kTB) {
      double r = b_own;
      for (int q0 = 0; q0 < sc; q0 += 16) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u)
          v[u] = q0 + u < sc ? ld_sc1(p.chol + L.fc + ((size_t)J * T + S[so + q0 + u]) * kTB + t) : 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (q0 + u < sc) r -= v[u];
      }
      rv[t] = r;
    }
    __syncthreads();
    // y_J[m] = sum_c L_JJ^-1[m][c] r[c]: thread (w, m) sums c in [16w, 16w + 16)
    double s3 = 0.0;
    for (int c = 16 * w; c < 16 * w + 16; ++c) s3 = __builtin_fma(VR[lane * kVR + c], rv[c], s3);
    part[w][lane] = s3;
    __syncthreads();
    if (t < kTB) yv[t] = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
    __syncthreads();
    for (int q = 0; q < rc; ++q) {
      const int I = S[ro + q];
      const double* LIJ = A + (size_t)(I * kTB + lane) * L.N + J * kTB + 16 * w;
      double la[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) la[c] = ld_sc1(LIJ + c);
      double s4 = 0.0;
#pragma unroll
      for (int c = 0; c < 16; ++c) s4 = __builtin_fma(la[c], yv[16 * w + c], s4);
      part[w][lane] = s4;
      __syncthreads();
      if (t < kTB)
        st_sc1(p.chol + L.fc + ((size_t)I * T + J) * kTB + t,
               ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t]);
      __syncthreads();
    }
    flow_publish(F.yf + J, epoch);
  }
  FLOW_T(4);
  // (4) back substitution: x_k = L_kk^-T (y_k - sum_I L_Ik^T x_I) over the row
  // tiles I of column k (thread (w, c = lane) sums rows [16w, 16w + 16) of every
  // I in row order; the operations and their order do not depend on which
  // workgroup forms x_k).  Who forms x_J:
  //   a root (no row tiles): this workgroup, right away;
  //   otherwise, once every workgroup of the grid has started (the start ticket
  //   reached T: waiting can then hold up no one), this workgroup registers as
  //   the waiter on cnt[J] (+2^16) and forms x_J when its row tiles' x are all
  //   retired -- unless the last of them was retired before it registered;
  //   else the workgroup that retires the last row tile of J (cnt[J] reaches
  //   rows(J) with no waiter registered) pushes J on its own stack.
  // So the columns run in parallel when the grid is resident, and a column whose
  // workgroup cannot wait is still formed.  Every column is retired once: x
  // flag, its children's counters, the retire ticket.
  if (t == 0) {
    sp_sh = 0;
    last_sh = 0;
    own_sh = 0;
    if (rc == 0) {
      own_sh = 1;
    } else if (ld_flag(F.start) >= epoch * T) {  // every workgroup of this solve has started
      const unsigned old = __hip_atomic_fetch_add(reinterpret_cast<unsigned*>(F.cnt + J), 1u << 16,
                                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      own_sh = (int)(old & 0xffffu) < rc ? 2 : 0;
    }
  }
  __syncthreads();
  if (!own_sh) {
    // another workgroup forms x_J: L_JJ^-1 and y_J for it, published by dv[J]
    double* V = p.chol + L.dinv + (size_t)J * kTB * kTB;
    for (int e = t; e < kTB * kTB; e += kTlWG) st_sc1(V + e, VR[(e >> 6) * kVR + (e & 63)]);
    if (t < kTB) st_sc1(p.chol + L.y + J * kTB + t, yv[t]);
    flow_publish(F.dv + J, epoch);
  }
  // the own column's first two L_IJ in flight before its wait (they are this
  // workgroup's own stores of (2)): only x_I is loaded after the counter
  double la_pre[2][16];
  if (own_sh == 2) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (q < rc) {
        const double* LIk = A + (size_t)(S[ro + q] * kTB + 16 * w) * L.N + J * kTB + lane;
#pragma unroll
        for (int m = 0; m < 16; ++m) la_pre[q][m] = ld_sc1(LIk + (size_t)m * L.N);
      }
  }
  for (int it = 0;; ++it) {
    int k;
    bool okk;
    if (it == 0) {  // this workgroup's own column, when it forms it
      if (!own_sh) continue;
      k = J;
      okk = ok && (own_sh == 1 || flow_wait_count(F.cnt + J, rc, epoch, fail, &shf));
    } else {
      if (t == 0) cur_sh = sp_sh > 0 ? stk[--sp_sh] : -1;
      __syncthreads();
      k = cur_sh;
      if (k < 0) break;
      okk = flow_wait(F.dv + k, epoch, fail, &shf);
    }
    const bool own = k == J;
    const int32_t* rk = S + S[5] + 5 * k;
    const int kro = rk[0], krc = rk[1], kso = rk[2], ksc = rk[3];
    // x_k's rows in camera order: loaded before the waits below, off the chain
    const int orow = own ? own_orow : (t < kTB ? tl_old_row(S, n, k * kTB + t) : -1);
    if (okk) {
      if (!own && t < kTB) yv[t] = ld_sc1(p.chol + L.y + k * kTB + t);
      double s2 = 0.0;
      for (int q = 0; q < krc; ++q) {
        const int I = S[kro + q];
        const double* LIk = A + (size_t)(I * kTB + 16 * w) * L.N + k * kTB + lane;
        const double* xI = p.chol + L.x + I * kTB + 16 * w;
        double la[16], xa[16];
        const bool pre = it == 0 && own_sh == 2 && q < 2;  // (uniform)
#pragma unroll
        for (int m = 0; m < 16; ++m) {
          la[m] = pre ? (q == 0 ? la_pre[0][m] : la_pre[1][m]) : ld_sc1(LIk + (size_t)m * L.N);
          xa[m] = ld_sc1(xI + m);
        }
#pragma unroll
        for (int m = 0; m < 16; ++m) s2 = __builtin_fma(la[m], xa[m], s2);
      }
      FLOW_TC(k, 5);
      part[w][lane] = s2;
      __syncthreads();
      if (t < kTB) rv[t] = yv[t] - (((part[0][t] + part[1][t]) + part[2][t]) + part[3][t]);
      __syncthreads();
      double s3 = 0.0;  // x_k[c] = sum_m L_kk^-1[m][c] r[m]
      if (own) {
        for (int m = 16 * w; m < 16 * w + 16; ++m) s3 = __builtin_fma(VR[m * kVR + lane], rv[m], s3);
      } else {
        const double* Vk = p.chol + L.dinv + (size_t)k * kTB * kTB;
        for (int m = 16 * w; m < 16 * w + 16; ++m) s3 = __builtin_fma(ld_sc1(Vk + m * kTB + lane), rv[m], s3);
      }
      __syncthreads();  // rv / part reads done before part is rewritten
      part[w][lane] = s3;
      __syncthreads();
      if (t < kTB) {
        const double xv = ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t];
        Xf[t] = xv;  // (4b) (Xf is free after (2))
        st_sc1(p.chol + L.x + k * kTB + t, xv);
        if (orow >= 0) st_sc1(p.chol + L.xo + orow, xv);  // camera order (padding rows dropped)
      }
    }
    // retire column k even when the solve failed (the counters and the ticket
    // still complete; the epilogue sees the fail code)
    flow_publish(F.xf + k, epoch);
    FLOW_TC(k, 6);
    // the parent counters (one lane each) in flight together -- independent,
    // and a chain of returning atomics cost a device round trip each on the
    // back substitution's critical path; the columns this retire completes go
    // on the stack in u order
    if (t < 64) {
      for (int u0 = 0; u0 == 0 || u0 < ksc; u0 += 64) {
        const int u = u0 + t;
        int c = 0, rcc = 0;
        unsigned old = 0;
        if (u < ksc) {
          c = S[kso + u];  // k is a row tile of column c
          rcc = S[S[5] + 5 * c + 1];
          old = ticket_add(reinterpret_cast<uint32_t*>(F.cnt + c));
        }
        const bool push = u < ksc && (int)(old & 0xffffu) == rcc - 1 && (old >> 16) == 0;
        const unsigned long long m = __ballot(push);
        const int base = sp_sh;
        if (push) stk[base + __popcll(m & ((1ull << t) - 1ull))] = c;
        wave_lds_fence();
        if (t == 0) sp_sh = base + __popcll(m);
        wave_lds_fence();
      }
    }
    // (4b) the epilogue of the cameras tile k owns (ba.tl_schedule: those whose
    // lowest tile is k -- every other tile of a camera is a row tile of k, so
    // its x is already out), after the retire so that no child waits on it:
    // delta_c, the trial parameters cams[1-cur] and their projection records,
    // this tile's share of the camera part of the predicted reduction and of
    // the cost (fixed order) into epi[k]; the same operations whichever
    // workgroup forms x_k.  Written through (sc1) and drained before the retire
    // ticket, so that the last retirer's failure path overwrites them safely.
    {
      const bool mine = own && own_sh != 0;
      const int32_t* er = S + S[7] + 2 * k;
      const int eo = mine ? e_off : er[0], ec = mine ? e_cnt : er[1];
      double* ct = Xf + kTB;                  // trial parameters [ec][9]
      double* pv = ct + 9 * kEpiCams;         // pc terms [9 ec]
      double* cv = pv + 9 * kEpiCams;         // cost terms [ec]
      if (t < 9 * ec) {
        int row = e_row, rn = e_rn;
        double cam = e_cam, du = e_du, g = e_g;
        if (!mine) {
          row = 9 * S[eo + t / 9] + t % 9;
          rn = tl_new_row(S, row);
          cam = p.cams[cur][row];
          g = bvec[n + row];
          du = bvec[2 * n + row];
        }
        const double d = (rn >> 6) == k ? Xf[rn & 63] : ld_sc1(p.chol + L.xo + row);
        st_sc1(p.delta_c + row, d);
        const double tr = cam + d;
        st_sc1(p.cams[1 - cur] + row, tr);
        ct[t] = tr;
        pv[t] = d * (lam * clampd(du) * d + g);
      }
      if (t < ec) cv[t] = mine ? e_cost : bvec[3 * n + S[eo + t]];
      __syncthreads();
      if (t < ec) {
        double rec[kCamRec];
        cam_prep(ct + 9 * t, rec);
        double* o = p.camrec[1 - cur] + kCamRec * S[eo + t];
#pragma unroll
        for (int i = 0; i < kCamRec; ++i) st_sc1(o + i, rec[i]);
      }
      if (t == 0) {
        double pc = 0.0, cs = 0.0;
        for (int i = 0; i < 9 * ec; ++i) pc += pv[i];
        for (int q = 0; q < ec; ++q) cs += cv[q];
        st_sc1(p.chol + L.epi + 2 * k, pc);
        st_sc1(p.chol + L.epi + 2 * k + 1, cs);
      }
      __builtin_amdgcn_s_waitcnt(0);
      __syncthreads();
      // (never reset: T retires per solve, the last of each solve is T - 1 mod T)
      if (t == 0 && ticket_add(reinterpret_cast<uint32_t*>(F.ticket)) % (unsigned)T == (unsigned)(T - 1))
        last_sh = 1;
    }
    __syncthreads();
  }
  FLOW_FLUSH();
  // (5) the workgroup that retired the last column (after its epilogue share)
  // sums the per-tile partials in tile order; after a failed solve it redoes
  // the whole epilogue with a zero step instead (its plain stores land after
  // the shares' drained write-through stores)
  if (!last_sh) return;
#ifdef SLAM_FLOW_PROFILE
  if (t == 0) g_flow_epi[0] = wall_clock64();
#endif
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const int fcode = flow_fcode(fail, epoch);  // 0 ok, 1 non-SPD tile, 2 a wait timed out
  if (fcode != 0) {
    const double* gvec = bvec + n;
    solve_epilogue<true>(p, p.chol + L.xo, false, &part[0][0],
                         EpiSrc{gvec, bvec + 2 * n, p.cams[cur], gvec + 2 * n}, fcode);
  } else if (t < 64) {
    double pc = 0.0, cs = 0.0;  // lane t: tiles t, t + 64, ...; then a fixed shuffle tree
    for (int k = t; k < T; k += 64) {
      pc += ld_sc1(p.chol + L.epi + 2 * k);
      cs += ld_sc1(p.chol + L.epi + 2 * k + 1);
    }
    for (int off = 32; off > 0; off >>= 1) {
      pc += __shfl_down(pc, off, 64);
      cs += __shfl_down(cs, off, 64);
    }
    if (t == 0) {
      p.state[SLAM_BA_ST_COST] = 0.5 * cs;
      p.state[SLAM_BA_ST_PRED_CAM] = 0.5 * pc;
      p.state[SLAM_BA_ST_CHOL_FAIL] = 0.0;
    }
  }
#ifdef SLAM_FLOW_PROFILE
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (t == 0) g_flow_epi[3] = wall_clock64();
#endif
  FLOW_TC(J, 7);
}

// The dataflow solve makes no residency assumption (k_tl3_flow's comment), so it
// runs on any stream, CU-masked or not, beside any other work.  It needs the
// column count within its LDS stack (SLAM_TL_FLOW_MAX_T, < 2^16 for the parent
// counters) and the camera-order x of the epilogue in its LDS scratch;
// otherwise (or with tl_mode "levels") the level-scheduled launches run.
static bool tl_flow_ok(const slam_ba_problem& p, hipStream_t) {
  if (p.tl_mode != 0 || p.tl_sched_host == nullptr || p.tl_sched_host[5] <= 0) return false;
  const TlLayout L(9 * p.n_cams, p.tl_sched_host[1]);
  return L.T <= SLAM_TL_FLOW_MAX_T && 9 * p.n_cams <= 2 * kTB * kTB;
}

// k_tl2_load over the structural tiles when the schedule carries the column table
static void tl_load(const slam_ba_problem& p, hipStream_t s) {
  const int32_t* h = p.tl_sched_host;
  const int T = h[1];
  if (h[5] > 0) {
    int maxrc = 0;
    for (int J = 0; J < T; ++J) maxrc = std::max(maxrc, (int)h[h[5] + 5 * J + 1]);
    k_tl2_load<<<dim3(T, 1 + maxrc), kTlWG, 0, s>>>(p, T, 1);
  } else {
    k_tl2_load<<<T * (T + 1) / 2, kTlWG, 0, s>>>(p, T, 0);
  }
}

// the layout the kernels assume (row maps at fixed offsets after the header,
// every row of S in some tile)
static int tl_check_sched(const slam_ba_problem& p) {
  const int32_t* h = p.tl_sched_host;
  const int n = 9 * p.n_cams, T = h[1];
  SLAM_REQUIRE(T >= (n + kTB - 1) / kTB && h[2] == kTlHdr && h[3] == kTlHdr + n &&
                   h[6] == kTlHdr + n + T * kTB && h[8] > 0 && h[9] > 0 && h[10] > h[9] && h[11] >= 0,
               "slam_ba: tl_sched layout is not ba.tl_schedule's (T %d, offsets %d %d %d for n %d)", T,
               h[2], h[3], h[6], n);
  return SLAM_OK;
}

static int tl_solve_flow(const slam_ba_problem& p, hipStream_t s) {
  const TlLayout L(9 * p.n_cams, p.tl_sched_host[1]);
  if (int rc = tl_check_sched(p)) return rc;
  k_tl3_flow<<<L.T, kTlWG, 0, s>>>(p, L.T);  // gathers its tiles from the packed system itself
  SLAM_LAUNCHED("k_tl3_flow");
  return SLAM_OK;
}

static int tl_solve_levels(const slam_ba_problem& p, hipStream_t s) {
  const TlLayout L(9 * p.n_cams, p.tl_sched_host[1]);
  const int32_t* h = p.tl_sched_host;
  const int nlev = h[0], T = h[1];
  if (int rc = tl_check_sched(p)) return rc;
  const int32_t* tab = h + h[4];
  tl_load(p, s);
  k_tl2_scatter<<<p.n_blocks, 128, 0, s>>>(p, L.T);
  for (int lv = 0; lv < nlev; ++lv) {
    const int32_t* e = tab + 6 * lv;
    if (e[1] > 0) k_tl2_panel<<<e[1], kTlWG, 0, s>>>(p, T, e[0]);
    if (e[3] > 0) k_tl2_update<<<e[3], kTlWG, 0, s>>>(p, T, e[2]);
  }
  for (int lv = nlev - 1; lv >= 0; --lv) {
    const int32_t* e = tab + 6 * lv;
    if (e[5] > 0) k_tl2_back<<<e[5], kTlWG, 0, s>>>(p, T, e[4]);
  }
  k_tl2_unperm<<<T, kTB, 0, s>>>(p, T);
  k_tl2_epilogue<<<1, 1024, 0, s>>>(p, T);
  SLAM_LAUNCHED("k_tl2_*");
  return SLAM_OK;
}

}  // namespace

// The camera solve of a packed system (9C > kLdsMaxN): the dataflow launch
// where tl_flow_ok allows it, the level-scheduled launches otherwise.
int slam::launch_solve_tiled(const slam_ba_problem& p, hipStream_t s) {
  return tl_flow_ok(p, s) ? tl_solve_flow(p, s) : tl_solve_levels(p, s);
}

extern "C" long long slam_ba_chol_len(int n_cams, const int32_t* tl_sched_host) {
  // tiled factor workspace (9C > kLdsMaxN) for a schedule of tl_sched_host[1]
  // tiles and tl_sched_host[11] product slots; no schedule: the fewest 64-row
  // tiles that hold 9C rows, no slots
  if (n_cams <= 0) return 0;
  const int n = 9 * n_cams;
  if (tl_sched_host == nullptr) return TlLayout(n, (n + kTB - 1) / kTB).total;
  return TlLayout(n, tl_sched_host[1]).with_slots(tl_sched_host[11]);
}

#ifdef SLAM_FLOW_PROFILE
extern "C" int slam_flow_epi_stamps(unsigned long long* out4) {
  SLAM_HIP(hipDeviceSynchronize());
  SLAM_HIP(hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_flow_epi), 4 * sizeof(unsigned long long)));
  return SLAM_OK;
}
extern "C" int slam_flow_sub_stamps(unsigned long long* out, int n_cols) {
  SLAM_HIP(hipDeviceSynchronize());
  SLAM_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_flow_sub), (size_t)n_cols * 8 * sizeof(unsigned long long)));
  return SLAM_OK;
}
extern "C" int slam_flow_fac_stamps(unsigned long long* out16) {
  SLAM_HIP(hipDeviceSynchronize());
  SLAM_HIP(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_flow_fac), 16 * sizeof(unsigned long long)));
  return SLAM_OK;
}
extern "C" int slam_flow_stamps(unsigned long long* out, int n_cols) {
  SLAM_HIP(hipDeviceSynchronize());
  SLAM_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_flow_stamp), (size_t)n_cols * 8 * sizeof(unsigned long long)));
  return SLAM_OK;
}
#endif
