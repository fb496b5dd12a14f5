// Guided matching (search by projection): project the landmarks into a frame
// with its predicted pose, look for each landmark's descriptor only among the
// keypoints in a small window round the predicted pixel, give every keypoint
// to at most one landmark and write the matches as track rows.
//
//   k_project      one lane per (frame, landmark): pinhole projection in f64 in
//                  the operation order the header states, NaN uv when invalid;
//   k_kp_grid      one workgroup per frame: keypoints binned into square cells
//                  (count in LDS, wg_exscan of wg_scan.hpp, scatter) -> CSR index;
//   k_window_knn2  one 16-lane DPP row per query, four queries per wave and no
//                  workgroup barrier.  Cells are row-major, so the cells a
//                  window covers in one cell row are ONE contiguous run of
//                  cell_kp; 8 lanes stride that run (the other 8 take the next
//                  cell row at the same time), test the exact window
//                  predicate on x, y and only then read the 32-byte descriptor
//                  (8 xor + v_bcnt against the query in 8 VGPRs, min / med3 on
//                  the key dist << 16 | j); four xor-shuffle steps merge the row;
//   k_unique       one workgroup per frame: atomicMin of d1 << 22 | query into
//                  the owner array, losers cleared, keys decoded;
//   k_track_rows   one workgroup per frame: order-preserving compaction (the rank of
//                  wg_scan.hpp written out, its second barrier after the row stores).
// The result of the search is defined by the window predicate alone (the grid
// only prunes), and every key is unique, so nothing depends on the order in
// which candidates, lanes or atomics arrive.
#include "common.hpp"
#include "hamming_bits.hpp"
#include "wg_scan.hpp"

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kMaxCells = 16384;   // cell counters of one frame in LDS (64 KiB)
constexpr int kGridWG = 1024;
constexpr int kKnnWG = 256;        // 4 waves x 4 rows of 16 lanes: 16 queries
constexpr int kQPerWG = kKnnWG / 16;
constexpr int kItemWG = 1024;      // k_unique / k_track_rows: one workgroup per frame
constexpr int kQBits = 22;         // owner key = d1 << 22 | query (d1 <= 256, query < 2^20)
constexpr uint32_t kQMask = (1u << kQBits) - 1u;

__global__ __launch_bounds__(256) void k_project(
    const double* __restrict__ X, size_t x_item, const int32_t* __restrict__ nx_arr, int x_cap,
    const double* __restrict__ poses, const double* __restrict__ P, double W, double H,
    double margin, double min_depth, float2* __restrict__ uv, double* __restrict__ z) {
  const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= min(max(nx_arr[b], 0), x_cap)) return;
  const double* T = poses + 16 * (size_t)b;
  const double* x = X + b * x_item + 3 * (size_t)i;
  const double d0 = x[0] - T[3], d1 = x[1] - T[7], d2 = x[2] - T[11];
  double xc[3], h[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) xc[k] = T[k] * d0 + T[4 + k] * d1 + T[8 + k] * d2;
#pragma unroll
  for (int r = 0; r < 3; ++r)
    h[r] = P[4 * r] * xc[0] + P[4 * r + 1] * xc[1] + P[4 * r + 2] * xc[2] + P[4 * r + 3];
  const double u = h[0] / h[2], v = h[1] / h[2];
  const bool ok = xc[2] > min_depth && h[2] > 0.0 && margin <= u && u < W - margin &&
                  margin <= v && v < H - margin;
  const float nan = __builtin_nanf("");
  const size_t o = (size_t)b * x_cap + i;
  uv[o] = ok ? make_float2((float)u, (float)v) : make_float2(nan, nan);
  if (z) z[o] = xc[2];
}

// cell of a keypoint, -1 when it lies outside [0, W) x [0, H) (NaN included)
__device__ __forceinline__ int cell_of(float x, float y, float W, float H, float inv, int gw) {
  if (!(x >= 0.f && x < W && y >= 0.f && y < H)) return -1;
  return (int)(y * inv) * gw + (int)(x * inv);
}

__global__ __launch_bounds__(kGridWG) void k_kp_grid(
    const float* __restrict__ kp, const int32_t* __restrict__ nkp_arr, int kp_cap, float W,
    float H, float inv, int gw, int ncell, int32_t* __restrict__ cell_ptr,
    int32_t* __restrict__ cell_kp) {
  __shared__ int cnt[kMaxCells];  // counts, then the write cursor of every cell
  __shared__ int wtot[kGridWG / kWave];
  const int b = blockIdx.x, t = threadIdx.x;
  const int n = clamp_count(nkp_arr[b], kp_cap);
  kp += (size_t)b * kp_cap * 5;
  cell_ptr += (size_t)b * (ncell + 1);
  cell_kp += (size_t)b * kp_cap;
  for (int c = t; c < ncell; c += kGridWG) cnt[c] = 0;
  __syncthreads();
  for (int j = t; j < n; j += kGridWG) {
    const int c = cell_of(kp[5 * (size_t)j], kp[5 * (size_t)j + 1], W, H, inv, gw);
    if (c >= 0) atomicAdd(&cnt[c], 1);
  }
  __syncthreads();
  // exclusive scan: every thread owns `per` consecutive cells
  const int per = (ncell + kGridWG - 1) / kGridWG;
  const int c0 = min(t * per, ncell), c1 = min(c0 + per, ncell);
  int sum = 0;
  for (int c = c0; c < c1; ++c) sum += cnt[c];
  int total;
  int base = wg_exscan<kGridWG>(sum, wtot, total);
  for (int c = c0; c < c1; ++c) {
    const int k = cnt[c];
    cnt[c] = base;
    cell_ptr[c] = base;
    base += k;
  }
  if (t == 0) cell_ptr[ncell] = total;
  __syncthreads();
  for (int j = t; j < n; j += kGridWG) {
    const int c = cell_of(kp[5 * (size_t)j], kp[5 * (size_t)j + 1], W, H, inv, gw);
    if (c >= 0) cell_kp[atomicAdd(&cnt[c], 1)] = j;
  }
}

struct KnnArgs {
  const uint4* q;
  const float2* quv;
  const float* qr;
  const int32_t* nq;
  const uint4* t;
  const float* kp;
  const int32_t* nt;
  const int32_t* cell_ptr;
  const int32_t* cell_kp;
  int2* idx2;
  int2* dist2;
  uint8_t* good;
  size_t q_item;  // uint4 per batch item of q (0: shared)
  int q_cap, t_cap, gw, gh;
  float W, H, inv;
  int max_dist, ratio_num, ratio_den;
};

__global__ __launch_bounds__(kKnnWG) void k_window_knn2(const KnnArgs a) {
  const int b = blockIdx.y;
  const int qi = blockIdx.x * kQPerWG + (threadIdx.x >> 4), sub = threadIdx.x & 15;
  const int nq = min(max(a.nq[b], 0), a.q_cap);
  if (qi >= nq) return;  // whole 16-lane rows leave together: no barrier below
  const int nt = min(max(a.nt[b], 0), a.t_cap);
  const size_t o = (size_t)b * a.q_cap + qi;
  const float2 c = a.quv[o];
  const float r = a.qr[o];
  uint32_t k1 = kNone, k2 = kNone;
  if (isfinite(c.x) && isfinite(c.y) && r > 0.f) {
    // Cells that can hold a candidate.  The predicate below is evaluated in
    // f32 (rounded differences), so the cell range is widened by far more than
    // those roundings; it only has to be a superset.
    const float m = (fabsf(c.x) + fabsf(c.y) + r) * 0x1p-20f;
    const float x0 = c.x - r - m, x1 = c.x + r + m, y0 = c.y - r - m, y1 = c.y + r + m;
    if (x1 >= 0.f && x0 < a.W && y1 >= 0.f && y0 < a.H) {
      const int cx0 = (int)(fmaxf(x0, 0.f) * a.inv);
      const int cx1 = min((int)(fminf(x1, a.W) * a.inv), a.gw - 1);
      const int cy0 = (int)(fmaxf(y0, 0.f) * a.inv);
      const int cy1 = min((int)(fminf(y1, a.H) * a.inv), a.gh - 1);
      const uint4* qd = a.q + b * a.q_item + 2 * (size_t)qi;
      const uint4 qa = qd[0], qb = qd[1];
      const uint32_t qv[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
      const int32_t* cp = a.cell_ptr + (size_t)b * (a.gw * a.gh + 1);
      const int32_t* ck = a.cell_kp + (size_t)b * a.t_cap;
      const float* kp = a.kp + (size_t)b * a.t_cap * 5;
      const uint4* td = a.t + (size_t)b * a.t_cap * 2;
      // Lanes 0-7 take the even cell rows of the window, lanes 8-15 the odd
      // ones: a window of 2 r <= cell pixels covers two cell rows, whose
      // dependent load chains (offsets, index, x y, descriptor) then run side
      // by side instead of one after the other.
      for (int cy = cy0 + (sub >> 3); cy <= cy1; cy += 2) {
        // one contiguous run of cell_kp (clamped: a grid that was not built
        // for these keypoints must not lead out of the buffers)
        const int p0 = max(cp[cy * a.gw + cx0], 0);
        const int p1 = min(cp[cy * a.gw + cx1 + 1], a.t_cap);
        for (int p = p0 + (sub & 7); p < p1; p += 8) {
          const int j = ck[p];
          if ((unsigned)j >= (unsigned)nt) continue;
          const float kx = kp[5 * (size_t)j], ky = kp[5 * (size_t)j + 1];
          if (!(fabsf(kx - c.x) <= r && fabsf(ky - c.y) <= r)) continue;
          const uint4 x = td[2 * (size_t)j], y = td[2 * (size_t)j + 1];
          const uint32_t key = (hd8(qv, x, y) << 16) | (uint32_t)j;
          k2 = umed3(k1, k2, key);
          k1 = min(k1, key);
        }
      }
    }
  }
  // the 16 partial lists of the row (an invalid query's row holds kNone only)
#pragma unroll
  for (int off = 1; off < 16; off <<= 1)
    merge2(k1, k2, __shfl_xor(k1, off, kWave), __shfl_xor(k2, off, kWave));
  if (sub != 0) return;
  const bool h1 = k1 != kNone, h2 = k2 != kNone;
  int2 id, ds;
  id.x = h1 ? (int)(k1 & 0xFFFFu) : -1;
  ds.x = h1 ? (int)(k1 >> 16) : -1;
  id.y = h2 ? (int)(k2 & 0xFFFFu) : -1;
  ds.y = h2 ? (int)(k2 >> 16) : -1;
  a.idx2[o] = id;
  a.dist2[o] = ds;
  a.good[o] = (h1 && ds.x <= a.max_dist && (!h2 || a.ratio_den * ds.x < a.ratio_num * ds.y)) ? 1 : 0;
}

// The owner words are written, raced for and read back inside ONE workgroup:
// the races and the reads after them are workgroup-scope atomics ordered by the
// workgroup barriers, which is all the memory model asks for -- no agent-scope
// fence, so no L2 write-back between the phases.
__device__ __forceinline__ uint32_t load_wg(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__global__ __launch_bounds__(kItemWG) void k_unique(
    const int2* __restrict__ idx2, const int2* __restrict__ dist2, const uint8_t* __restrict__ good,
    const int32_t* __restrict__ nq_arr, int q_cap, int t_cap, uint32_t* owner,
    uint8_t* __restrict__ good_out) {
  const int b = blockIdx.x, t = threadIdx.x;
  const int nq = min(max(nq_arr[b], 0), q_cap);
  owner += (size_t)b * t_cap;
  const size_t qo = (size_t)b * q_cap;
  for (int j = t; j < t_cap; j += kItemWG)
    __hip_atomic_store(&owner[j], kNone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  for (int q = t; q < nq; q += kItemWG) {
    const int j = idx2[qo + q].x;
    if (good[qo + q] && (unsigned)j < (unsigned)t_cap)
      __hip_atomic_fetch_min(&owner[j], ((uint32_t)dist2[qo + q].x << kQBits) | (uint32_t)q,
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  for (int q = t; q < nq; q += kItemWG) {
    const int j = idx2[qo + q].x;
    const bool mine = good[qo + q] && (unsigned)j < (unsigned)t_cap &&
                      (load_wg(&owner[j]) & kQMask) == (uint32_t)q;
    good_out[qo + q] = mine ? 1 : 0;
  }
  __syncthreads();  // every read of the keys is done before they are decoded
  for (int j = t; j < t_cap; j += kItemWG) {
    const uint32_t k = load_wg(&owner[j]);
    owner[j] = k == kNone ? kNone : (k & kQMask);
  }
}

__global__ __launch_bounds__(kItemWG) void k_track_rows(
    const int2* __restrict__ idx2, const uint8_t* __restrict__ good,
    const int32_t* __restrict__ nq_arr, int q_cap, const float* __restrict__ kp, int kp_cap,
    int frame0, int rows_cap, double* __restrict__ rows, int32_t* __restrict__ count) {
  __shared__ int wave_tot[kItemWG / kWave];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & (kWave - 1), wid = t / kWave;
  const int nq = clamp_count(nq_arr[b], q_cap);
  const size_t qo = (size_t)b * q_cap;
  kp += (size_t)b * kp_cap * 5;
  rows += (size_t)b * rows_cap * 4;
  int carry = 0;  // rows written so far (uniform)
  for (int base = 0; base < nq; base += kItemWG) {
    const int q = base + t;
    int j = -1;
    if (q < nq && good[qo + q]) j = idx2[qo + q].x;
    const bool keep = (unsigned)j < (unsigned)kp_cap;
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wid] = __popcll(m);
    __syncthreads();
    int off = carry, tot = 0;
    for (int w = 0; w < kItemWG / kWave; ++w) {
      off += w < wid ? wave_tot[w] : 0;
      tot += wave_tot[w];
    }
    const int row = off + before;
    if (keep && row < rows_cap) {
      double* o = rows + 4 * (size_t)row;
      o[0] = (double)(frame0 + b);
      o[1] = (double)q;
      o[2] = (double)kp[5 * (size_t)j];
      o[3] = (double)kp[5 * (size_t)j + 1];
    }
    carry += tot;
    __syncthreads();  // wave_tot reuse
  }
  if (t == 0) count[b] = min(carry, rows_cap);
}

bool cell_ok(int cell) { return cell == 16 || cell == 32 || cell == 64; }

}  // namespace

extern "C" int slam_project_landmarks(const double* d_X, int x_shared, const int32_t* d_nx,
                                      int x_cap, int batch, const double* d_poses,
                                      const double* d_P, int W, int H, double margin,
                                      double min_depth, float* d_uv, double* d_z, void* stream) {
  SLAM_REQUIRE(batch >= 0 && x_cap >= 0, "slam_project_landmarks: bad shape");
  SLAM_REQUIRE(W > 0 && H > 0, "slam_project_landmarks: image size %d x %d", W, H);
  SLAM_REQUIRE(margin >= 0.0, "slam_project_landmarks: margin must be >= 0");  // NaN refused too
  SLAM_REQUIRE(min_depth == min_depth, "slam_project_landmarks: min_depth is NaN");
  if (batch == 0 || x_cap == 0) return SLAM_OK;
  SLAM_REQUIRE(d_X && d_nx && d_poses && d_P && d_uv, "slam_project_landmarks: null pointer");
  SLAM_REQUIRE(batch <= 65535, "slam_project_landmarks: batch %d > 65535", batch);
  k_project<<<dim3(nblk(x_cap, 256), batch), 256, 0, slam::as_stream(stream)>>>(
      d_X, x_shared ? 0 : (size_t)x_cap * 3, d_nx, x_cap, d_poses, d_P, (double)W, (double)H,
      margin, min_depth, reinterpret_cast<float2*>(d_uv), d_z);
  SLAM_LAUNCHED("k_project");
  return SLAM_OK;
}

extern "C" int slam_kp_grid(const float* d_kp, const int32_t* d_nkp, int kp_cap, int batch, int W,
                            int H, int cell, int32_t* d_cell_ptr, int32_t* d_cell_kp,
                            void* stream) {
  SLAM_REQUIRE(batch >= 0 && kp_cap >= 0, "slam_kp_grid: bad shape");
  SLAM_REQUIRE(W > 0 && H > 0, "slam_kp_grid: image size %d x %d", W, H);
  SLAM_REQUIRE(cell_ok(cell), "slam_kp_grid: cell %d is not 16, 32 or 64", cell);
  SLAM_REQUIRE(kp_cap <= 65535, "slam_kp_grid: kp_cap %d > 65535", kp_cap);
  const long long gw = (W + cell - 1) / cell, gh = (H + cell - 1) / cell;
  SLAM_REQUIRE(gw * gh <= kMaxCells, "slam_kp_grid: grid %lld x %lld cells > %d (use a larger cell)",
               gw, gh, kMaxCells);
  if (batch == 0) return SLAM_OK;
  SLAM_REQUIRE(d_nkp && d_cell_ptr && (kp_cap == 0 || (d_kp && d_cell_kp)),
               "slam_kp_grid: null pointer");
  k_kp_grid<<<batch, kGridWG, 0, slam::as_stream(stream)>>>(
      d_kp, d_nkp, kp_cap, (float)W, (float)H, 1.0f / (float)cell, (int)gw, (int)(gw * gh),
      d_cell_ptr, d_cell_kp);
  SLAM_LAUNCHED("k_kp_grid");
  return SLAM_OK;
}

extern "C" int slam_hamming_window_knn2(const uint8_t* d_q, int q_shared, const float* d_quv,
                                        const float* d_qr, const int32_t* d_nq, int q_cap,
                                        const uint8_t* d_t, const float* d_kp,
                                        const int32_t* d_nt, int t_cap,
                                        const int32_t* d_cell_ptr, const int32_t* d_cell_kp, int W,
                                        int H, int cell, int batch, int max_dist, int ratio_num,
                                        int ratio_den, int32_t* d_idx2, int32_t* d_dist2,
                                        uint8_t* d_good, void* stream) {
  SLAM_REQUIRE(batch >= 0 && q_cap >= 0 && t_cap >= 0, "slam_hamming_window_knn2: bad shape");
  SLAM_REQUIRE(t_cap <= 65535, "slam_hamming_window_knn2: t_cap %d > 65535", t_cap);
  SLAM_REQUIRE(q_cap <= (1 << 20), "slam_hamming_window_knn2: q_cap %d > 1 << 20", q_cap);
  SLAM_REQUIRE(W > 0 && H > 0, "slam_hamming_window_knn2: image size %d x %d", W, H);
  SLAM_REQUIRE(cell_ok(cell), "slam_hamming_window_knn2: cell %d is not 16, 32 or 64", cell);
  const long long gw = (W + cell - 1) / cell, gh = (H + cell - 1) / cell;
  SLAM_REQUIRE(gw * gh <= kMaxCells, "slam_hamming_window_knn2: grid %lld x %lld cells > %d", gw,
               gh, kMaxCells);
  SLAM_REQUIRE(max_dist >= 0 && max_dist <= 256, "slam_hamming_window_knn2: max_dist %d not in 0..256",
               max_dist);
  SLAM_REQUIRE(ratio_num > 0 && ratio_num <= ratio_den && ratio_den <= (1 << 20),
               "slam_hamming_window_knn2: ratio %d / %d needs 0 < num <= den <= 1 << 20", ratio_num,
               ratio_den);
  if (batch == 0 || q_cap == 0) return SLAM_OK;
  SLAM_REQUIRE(d_q && d_quv && d_qr && d_nq && d_nt && d_cell_ptr && d_idx2 && d_dist2 && d_good &&
                   (t_cap == 0 || (d_t && d_kp && d_cell_kp)),
               "slam_hamming_window_knn2: null pointer");
  SLAM_REQUIRE(((uintptr_t)d_q & 15) == 0 && ((uintptr_t)d_t & 15) == 0,
               "slam_hamming_window_knn2: descriptor buffers must be 16-byte aligned");
  SLAM_REQUIRE(batch <= 65535, "slam_hamming_window_knn2: batch %d > 65535", batch);
  KnnArgs a;
  a.q = reinterpret_cast<const uint4*>(d_q);
  a.quv = reinterpret_cast<const float2*>(d_quv);
  a.qr = d_qr;
  a.nq = d_nq;
  a.t = reinterpret_cast<const uint4*>(d_t);
  a.kp = d_kp;
  a.nt = d_nt;
  a.cell_ptr = d_cell_ptr;
  a.cell_kp = d_cell_kp;
  a.idx2 = reinterpret_cast<int2*>(d_idx2);
  a.dist2 = reinterpret_cast<int2*>(d_dist2);
  a.good = d_good;
  a.q_item = q_shared ? 0 : (size_t)q_cap * 2;
  a.q_cap = q_cap;
  a.t_cap = t_cap;
  a.gw = (int)gw;
  a.gh = (int)gh;
  a.W = (float)W;
  a.H = (float)H;
  a.inv = 1.0f / (float)cell;
  a.max_dist = max_dist;
  a.ratio_num = ratio_num;
  a.ratio_den = ratio_den;
  k_window_knn2<<<dim3(nblk(q_cap, kQPerWG), batch), kKnnWG, 0, slam::as_stream(stream)>>>(a);
  SLAM_LAUNCHED("k_window_knn2");
  return SLAM_OK;
}

extern "C" int slam_match_unique(const int32_t* d_idx2, const int32_t* d_dist2,
                                 const uint8_t* d_good, const int32_t* d_nq, int q_cap, int t_cap,
                                 int batch, int32_t* d_owner, uint8_t* d_good_out, void* stream) {
  SLAM_REQUIRE(batch >= 0 && q_cap >= 0 && t_cap >= 0, "slam_match_unique: bad shape");
  SLAM_REQUIRE(t_cap <= 65535, "slam_match_unique: t_cap %d > 65535", t_cap);
  SLAM_REQUIRE(q_cap <= (1 << 20), "slam_match_unique: q_cap %d > 1 << 20", q_cap);
  if (batch == 0) return SLAM_OK;
  SLAM_REQUIRE(d_nq && (q_cap == 0 || (d_idx2 && d_dist2 && d_good && d_good_out)) &&
                   (t_cap == 0 || d_owner),
               "slam_match_unique: null pointer");
  k_unique<<<batch, kItemWG, 0, slam::as_stream(stream)>>>(
      reinterpret_cast<const int2*>(d_idx2), reinterpret_cast<const int2*>(d_dist2), d_good, d_nq,
      q_cap, t_cap, reinterpret_cast<uint32_t*>(d_owner), d_good_out);
  SLAM_LAUNCHED("k_unique");
  return SLAM_OK;
}

extern "C" int slam_track_rows(const int32_t* d_idx2, const uint8_t* d_good, const int32_t* d_nq,
                               int q_cap, const float* d_kp, int kp_cap, int batch, int frame0,
                               int rows_cap, double* d_rows, int32_t* d_count, void* stream) {
  SLAM_REQUIRE(batch >= 0 && q_cap >= 0 && kp_cap >= 0 && rows_cap >= 0,
               "slam_track_rows: bad shape");
  SLAM_REQUIRE(rows_cap >= (q_cap < kp_cap ? q_cap : kp_cap),
               "slam_track_rows: rows_cap %d < min(q_cap %d, kp_cap %d)", rows_cap, q_cap, kp_cap);
  if (batch == 0) return SLAM_OK;
  const bool any = q_cap > 0 && kp_cap > 0;
  SLAM_REQUIRE(d_nq && d_count && (!any || (d_idx2 && d_good && d_kp && d_rows)),
               "slam_track_rows: null pointer");
  k_track_rows<<<batch, kItemWG, 0, slam::as_stream(stream)>>>(
      reinterpret_cast<const int2*>(d_idx2), d_good, d_nq, q_cap, d_kp, kp_cap, frame0, rows_cap,
      d_rows, d_count);
  SLAM_LAUNCHED("k_track_rows");
  return SLAM_OK;
}
