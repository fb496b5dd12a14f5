// Relocalization against a device-resident map (include/slam355.h,
// "Relocalization"): a pose from the map without a prior.
//
//   k_map_knn2_part   Hamming kNN-2 of a frame's keypoints against ONE segment
//                     of kSeg landmarks.  Grid = (query tile, segment, item), so
//                     one frame against a large map still fills the chip.  The
//                     inner loop is knn2_kernel's (hamming.hip): a workgroup is
//                     128 queries held in VGPRs by each of its 8 waves, a wave
//                     takes every 8th landmark of the segment, the descriptor
//                     comes through scalar loads and the running top-2 is min /
//                     med3 on dist << 16 | segment-local index.  Eligibility
//                     (alive, inside the map's count, last in [lo, hi)) is
//                     scalar work once per landmark and wave, next to the
//                     descriptor load -- not per query: an ineligible landmark's
//                     index operand is all ones, so its key is kNone whatever
//                     the distance and costs no extra VALU instruction.  The
//                     workgroup writes its queries' top-2 as dist << 20 | global
//                     index: the segment offset is added here, not in the loop;
//   k_map_knn2_merge  one lane per query: min / med3 over the segments'
//                     partials (keys are unique, so the order is immaterial),
//                     decode, ratio test;
//   k_reloc_rows      one workgroup per frame: the landmarks that own a keypoint,
//                     ranked by ballot + wave totals (k_track_rows), written as
//                     track rows and as PnP's object / image points;
//   k_reloc_pose      one lane per frame: PnP's (rvec, tvec) -> the camera-to-world
//                     start pose of the refinement, or the prior.
// Nothing here waits for another workgroup: what one launch leaves for the
// next goes through memory and the launch boundary.
#include "common.hpp"
#include "hamming_bits.hpp"
#include "pose_math.hpp"
#include "wg_scan.hpp"

namespace {

constexpr int kSeg = SLAM_MAP_KNN_SEGMENT;  // landmarks per segment
constexpr int kWG = 512;
constexpr int kWaves = kWG / kWave;      // 8: the landmarks of a segment are dealt over the waves
constexpr int kQPL = 2;                  // queries per lane
constexpr int kQPerWG = kWave * kQPL;    // 128 queries per workgroup (every wave holds all of them)
constexpr int kRowsAhead = 8;            // landmarks loaded ahead per wave
constexpr int kMergeWG = 256;
constexpr int kItemWG = 1024;            // k_reloc_rows: one workgroup per frame
constexpr int kIdxBits = 20;             // partial key = dist << 20 | landmark (< 1 << 20)
constexpr uint32_t kIdxMask = (1u << kIdxBits) - 1u;
constexpr uint32_t kNone = 0xFFFFFFFFu;
static_assert(kSeg >= kWaves && kSeg <= 65536, "the loop's key holds a 16-bit segment-local index");

__global__ __launch_bounds__(kWG) void k_map_knn2_part(
    const uint4* __restrict__ q, const int32_t* __restrict__ nq_arr, int q_cap,
    const uint4* __restrict__ desc, const uint2* __restrict__ X, const int32_t* __restrict__ last,
    const int32_t* __restrict__ n_ptr, int x_cap, const int2* __restrict__ range, int nseg,
    uint2* __restrict__ part) {
  __shared__ uint32_t lds[kWaves][2][kQPerWG];
  const int tile = blockIdx.x, seg = blockIdx.y, item = blockIdx.z;
  const int nq = clamp_count(nq_arr[item], q_cap);
  const int nt = clamp_count(*n_ptr, x_cap);
  const int q0 = tile * kQPerWG, r0 = seg * kSeg;
  if (q0 >= nq || r0 >= nt) return;  // uniform over the workgroup; the merge reads neither
  const int r1 = min(r0 + kSeg, nt);
  const int2 lh = range[item];
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);  // uniform: scalar loop

  const uint4* qb = q + (size_t)item * q_cap * 2;
  uint32_t qa[kQPL][8];
  uint32_t k1[kQPL], k2[kQPL];
#pragma unroll
  for (int s = 0; s < kQPL; ++s) {
    const int qi = q0 + s * kWave + lane;
    uint4 a = make_uint4(0, 0, 0, 0), b = a;
    if (qi < nq) {
      a = qb[2 * qi];
      b = qb[2 * qi + 1];
    }
    qa[s][0] = a.x; qa[s][1] = a.y; qa[s][2] = a.z; qa[s][3] = a.w;
    qa[s][4] = b.x; qa[s][5] = b.y; qa[s][6] = b.z; qa[s][7] = b.w;
    k1[s] = kNone;
    k2[s] = kNone;
  }

  // the index operand of landmark i's key: its segment-local index, or all ones
  // when it is not eligible (dist << 16 | all ones = kNone).  i is uniform: the
  // words of X[i][0] and last[i] come through the scalar cache like the descriptor.
  auto index_or_none = [&](int i) -> uint32_t {
    const uint2 x = X[3 * (size_t)i];  // the bits of X[i][0]
    const int l = last[i];
    const uint32_t h = x.y & 0x7FFFFFFFu;
    const bool nan = h > 0x7FF00000u || (h == 0x7FF00000u && x.x != 0u);
    return (!nan && l >= lh.x && l < lh.y) ? (uint32_t)(i - r0) : kNone;
  };

  int j = r0 + wid;
  for (; j + (kRowsAhead - 1) * kWaves < r1; j += kRowsAhead * kWaves) {
    uint4 x[kRowsAhead], y[kRowsAhead];
    uint32_t jj[kRowsAhead];
#pragma unroll
    for (int u = 0; u < kRowsAhead; ++u) {
      x[u] = desc[2 * (size_t)(j + u * kWaves)];
      y[u] = desc[2 * (size_t)(j + u * kWaves) + 1];
      jj[u] = index_or_none(j + u * kWaves);
    }
#pragma unroll
    for (int u = 0; u < kRowsAhead; ++u) {
#pragma unroll
      for (int s = 0; s < kQPL; ++s) {
        const uint32_t key = (hd8(qa[s], x[u], y[u]) << 16) | jj[u];
        k2[s] = umed3(k1[s], k2[s], key);
        k1[s] = min(k1[s], key);
      }
    }
  }
  for (; j < r1; j += kWaves) {
    const uint4 x = desc[2 * (size_t)j];
    const uint4 y = desc[2 * (size_t)j + 1];
    const uint32_t jj = index_or_none(j);
#pragma unroll
    for (int s = 0; s < kQPL; ++s) {
      const uint32_t key = (hd8(qa[s], x, y) << 16) | jj;
      k2[s] = umed3(k1[s], k2[s], key);
      k1[s] = min(k1[s], key);
    }
  }
  // merge the wave partials
#pragma unroll
  for (int s = 0; s < kQPL; ++s) {
    lds[wid][0][s * kWave + lane] = k1[s];
    lds[wid][1][s * kWave + lane] = k2[s];
  }
  __syncthreads();
  if (threadIdx.x >= kQPerWG) return;
  const int ql = threadIdx.x;
  const int qi = q0 + ql;
  if (qi >= nq) return;
  uint32_t m1 = lds[0][0][ql], m2 = lds[0][1][ql];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) merge2(m1, m2, lds[w][0][ql], lds[w][1][ql]);
  // segment-local keys -> global ones: the same order inside the segment, and
  // across segments (distance, then landmark index) as well
  const uint32_t g1 = m1 == kNone ? kNone : ((m1 >> 16) << kIdxBits) | (uint32_t)(r0 + (int)(m1 & 0xFFFFu));
  const uint32_t g2 = m2 == kNone ? kNone : ((m2 >> 16) << kIdxBits) | (uint32_t)(r0 + (int)(m2 & 0xFFFFu));
  part[((size_t)item * nseg + seg) * q_cap + qi] = make_uint2(g1, g2);
}

__global__ __launch_bounds__(kMergeWG) void k_map_knn2_merge(
    const uint2* __restrict__ part, const int32_t* __restrict__ nq_arr, int q_cap,
    const int32_t* __restrict__ n_ptr, int x_cap, int nseg, int max_dist, int ratio_num,
    int ratio_den, int2* __restrict__ idx2, int2* __restrict__ dist2, uint8_t* __restrict__ good) {
  const int item = blockIdx.y, qi = blockIdx.x * kMergeWG + threadIdx.x;
  if (qi >= clamp_count(nq_arr[item], q_cap)) return;
  const int live = (clamp_count(*n_ptr, x_cap) + kSeg - 1) / kSeg;  // the segments that wrote (<= nseg)
  uint32_t m1 = kNone, m2 = kNone;
  const uint2* p = part + (size_t)item * nseg * q_cap + qi;
  for (int s = 0; s < live; ++s) {
    const uint2 a = p[(size_t)s * q_cap];
    merge2(m1, m2, a.x, a.y);
  }
  const bool h1 = m1 != kNone, h2 = m2 != kNone;
  int2 id, ds;
  id.x = h1 ? (int)(m1 & kIdxMask) : -1;
  ds.x = h1 ? (int)(m1 >> kIdxBits) : -1;
  id.y = h2 ? (int)(m2 & kIdxMask) : -1;
  ds.y = h2 ? (int)(m2 >> kIdxBits) : -1;
  const size_t o = (size_t)item * q_cap + qi;
  idx2[o] = id;
  dist2[o] = ds;
  good[o] = (h2 && ds.x <= max_dist && ratio_den * ds.x < ratio_num * ds.y) ? 1 : 0;
}

__global__ __launch_bounds__(kItemWG) void k_reloc_rows(
    const int32_t* __restrict__ owner, const int32_t* __restrict__ n_ptr, int x_cap,
    const float* __restrict__ kp, int kp_cap, const double* __restrict__ X, int frame0,
    int rows_cap, double* __restrict__ rows, int32_t* __restrict__ count, double* __restrict__ Q,
    double* __restrict__ q) {
  __shared__ int wave_tot[kItemWG / kWave];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & (kWave - 1), wid = t / kWave;
  const int n = clamp_count(*n_ptr, x_cap);
  owner += (size_t)b * x_cap;
  kp += (size_t)b * kp_cap * 5;
  rows += (size_t)b * rows_cap * 4;
  Q += (size_t)b * rows_cap * 3;
  q += (size_t)b * rows_cap * 2;
  int carry = 0;  // rows written so far (uniform)
  for (int base = 0; base < n; base += kItemWG) {
    const int i = base + t;
    const int j = i < n ? owner[i] : -1;
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
      const double kx = (double)kp[5 * (size_t)j], ky = (double)kp[5 * (size_t)j + 1];
      double* o = rows + 4 * (size_t)row;
      o[0] = (double)(frame0 + b);
      o[1] = (double)i;
      o[2] = kx;
      o[3] = ky;
      Q[3 * (size_t)row] = X[3 * (size_t)i];
      Q[3 * (size_t)row + 1] = X[3 * (size_t)i + 1];
      Q[3 * (size_t)row + 2] = X[3 * (size_t)i + 2];
      q[2 * (size_t)row] = kx;
      q[2 * (size_t)row + 1] = ky;
    }
    carry += tot;
    __syncthreads();  // wave_tot reuse
  }
  if (t == 0) count[b] = min(carry, rows_cap);
}

__global__ __launch_bounds__(kWave) void k_reloc_pose(
    const double* __restrict__ rvec, const double* __restrict__ tvec,
    const int32_t* __restrict__ ninl, const int32_t* __restrict__ count,
    const double* __restrict__ P, const double* __restrict__ prior, int batch, int min_inliers,
    double* __restrict__ poses, int32_t* __restrict__ count_out) {
  const int b = blockIdx.x * kWave + threadIdx.x;
  if (b >= batch) return;
  double* T = poses + 16 * (size_t)b;
  if (ninl[b] < min_inliers) {
    for (int k = 0; k < 16; ++k) T[k] = prior ? prior[16 * (size_t)b + k] : (k % 5 == 0 ? 1.0 : 0.0);
    count_out[b] = 0;
    return;
  }
  // P = K [I | s]: s by back substitution through the upper triangular K
  const double s2 = P[11] / P[10];
  const double s1 = (P[7] - P[6] * s2) / P[5];
  const double s0 = ((P[3] - P[1] * s1) - P[2] * s2) / P[0];
  double R[9];
  rodrigues(rvec + 3 * (size_t)b, R);
  const double d0 = tvec[3 * (size_t)b] - s0, d1 = tvec[3 * (size_t)b + 1] - s1,
               d2 = tvec[3 * (size_t)b + 2] - s2;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[4 * r + c] = R[3 * c + r];
    T[4 * r + 3] = -((R[r] * d0 + R[3 + r] * d1) + R[6 + r] * d2);
  }
  T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
  count_out[b] = count[b];
}

size_t knn2_ws_bytes(int batch, int q_cap, int x_cap) {
  const size_t nseg = (size_t)((x_cap + kSeg - 1) / kSeg);
  return (size_t)batch * nseg * (size_t)q_cap * sizeof(uint2);
}

bool knn2_shape_ok(const char* fn, int batch, int q_cap, int x_cap) {
  if (!(batch >= 1 && batch <= 65535)) {
    slam::set_error("%s: batch %d not in 1..65535", fn, batch);
    return false;
  }
  if (!(q_cap >= 1 && q_cap <= 65535)) {
    slam::set_error("%s: q_cap %d not in 1..65535", fn, q_cap);
    return false;
  }
  if (!(x_cap >= 1 && x_cap <= kMaxLandmarks)) {
    slam::set_error("%s: x_cap %d not in 1..%d", fn, x_cap, kMaxLandmarks);
    return false;
  }
  return true;
}

}  // namespace

extern "C" int slam_hamming_map_segment(void) { return kSeg; }

extern "C" int slam_hamming_map_workspace_bytes(int batch, int q_cap, int x_cap, size_t* bytes) {
  if (!knn2_shape_ok("slam_hamming_map_workspace_bytes", batch, q_cap, x_cap)) return SLAM_ERR_ARG;
  NEED("slam_hamming_map_workspace_bytes", bytes);
  *bytes = knn2_ws_bytes(batch, q_cap, x_cap);
  return SLAM_OK;
}

extern "C" int slam_hamming_map_knn2(const uint8_t* d_q, const int32_t* d_nq, int q_cap,
                                     const uint8_t* d_desc, const double* d_X,
                                     const int32_t* d_last, const int32_t* d_n, int x_cap,
                                     const int32_t* d_range, int batch, int max_dist,
                                     int ratio_num, int ratio_den, int32_t* d_idx2,
                                     int32_t* d_dist2, uint8_t* d_good, void* d_ws,
                                     size_t ws_bytes, void* stream) {
  if (!knn2_shape_ok("slam_hamming_map_knn2", batch, q_cap, x_cap)) return SLAM_ERR_ARG;
  SLAM_REQUIRE(max_dist >= 0 && max_dist <= 256, "slam_hamming_map_knn2: max_dist %d not in 0..256",
               max_dist);
  SLAM_REQUIRE(ratio_num > 0 && ratio_num <= ratio_den && ratio_den <= (1 << 20),
               "slam_hamming_map_knn2: ratio %d / %d needs 0 < num <= den <= 1 << 20", ratio_num,
               ratio_den);
  NEED("slam_hamming_map_knn2", d_q);
  NEED("slam_hamming_map_knn2", d_nq);
  NEED("slam_hamming_map_knn2", d_desc);
  NEED("slam_hamming_map_knn2", d_X);
  NEED("slam_hamming_map_knn2", d_last);
  NEED("slam_hamming_map_knn2", d_n);
  NEED("slam_hamming_map_knn2", d_range);
  NEED("slam_hamming_map_knn2", d_idx2);
  NEED("slam_hamming_map_knn2", d_dist2);
  NEED("slam_hamming_map_knn2", d_good);
  NEED("slam_hamming_map_knn2", d_ws);
  NEED_ALIGNED16("slam_hamming_map_knn2", d_q);
  NEED_ALIGNED16("slam_hamming_map_knn2", d_desc);
  SLAM_REQUIRE(((uintptr_t)d_ws & 7) == 0, "slam_hamming_map_knn2: d_ws must be 8-byte aligned");
  SLAM_REQUIRE(ws_bytes >= knn2_ws_bytes(batch, q_cap, x_cap),
               "slam_hamming_map_knn2: ws_bytes %zu < %zu", ws_bytes,
               knn2_ws_bytes(batch, q_cap, x_cap));
  const int nseg = (x_cap + kSeg - 1) / kSeg;
  uint2* part = reinterpret_cast<uint2*>(d_ws);
  k_map_knn2_part<<<dim3(nblk(q_cap, kQPerWG), nseg, batch), kWG, 0, slam::as_stream(stream)>>>(
      reinterpret_cast<const uint4*>(d_q), d_nq, q_cap, reinterpret_cast<const uint4*>(d_desc),
      reinterpret_cast<const uint2*>(d_X), d_last, d_n, x_cap,
      reinterpret_cast<const int2*>(d_range), nseg, part);
  SLAM_LAUNCHED("k_map_knn2_part");
  k_map_knn2_merge<<<dim3(nblk(q_cap, kMergeWG), batch), kMergeWG, 0, slam::as_stream(stream)>>>(
      part, d_nq, q_cap, d_n, x_cap, nseg, max_dist, ratio_num, ratio_den,
      reinterpret_cast<int2*>(d_idx2), reinterpret_cast<int2*>(d_dist2), d_good);
  SLAM_LAUNCHED("k_map_knn2_merge");
  return SLAM_OK;
}

extern "C" int slam_reloc_rows(const int32_t* d_owner, const int32_t* d_n, int x_cap,
                               const float* d_kp, int kp_cap, const double* d_X, int batch,
                               int frame0, int rows_cap, double* d_rows, int32_t* d_count,
                               double* d_Q, double* d_q, void* stream) {
  SLAM_REQUIRE(batch >= 1 && batch <= 65535, "slam_reloc_rows: batch %d not in 1..65535", batch);
  SLAM_REQUIRE(x_cap >= 1 && x_cap <= kMaxLandmarks, "slam_reloc_rows: x_cap %d not in 1..%d", x_cap,
               kMaxLandmarks);
  SLAM_REQUIRE(kp_cap >= 1 && kp_cap <= (1 << 20), "slam_reloc_rows: kp_cap %d not in 1..1 << 20",
               kp_cap);
  SLAM_REQUIRE(rows_cap >= (x_cap < kp_cap ? x_cap : kp_cap),
               "slam_reloc_rows: rows_cap %d < min(x_cap %d, kp_cap %d)", rows_cap, x_cap, kp_cap);
  NEED("slam_reloc_rows", d_owner);
  NEED("slam_reloc_rows", d_n);
  NEED("slam_reloc_rows", d_kp);
  NEED("slam_reloc_rows", d_X);
  NEED("slam_reloc_rows", d_rows);
  NEED("slam_reloc_rows", d_count);
  NEED("slam_reloc_rows", d_Q);
  NEED("slam_reloc_rows", d_q);
  k_reloc_rows<<<batch, kItemWG, 0, slam::as_stream(stream)>>>(
      d_owner, d_n, x_cap, d_kp, kp_cap, d_X, frame0, rows_cap, d_rows, d_count, d_Q, d_q);
  SLAM_LAUNCHED("k_reloc_rows");
  return SLAM_OK;
}

extern "C" int slam_reloc_pose(const double* d_rvec, const double* d_tvec, const int32_t* d_ninl,
                               const int32_t* d_count, const double* d_P, const double* d_prior,
                               int batch, int min_inliers, double* d_poses, int32_t* d_count_out,
                               void* stream) {
  SLAM_REQUIRE(batch >= 1 && batch <= 65535, "slam_reloc_pose: batch %d not in 1..65535", batch);
  SLAM_REQUIRE(min_inliers >= 0, "slam_reloc_pose: min_inliers %d < 0", min_inliers);
  NEED("slam_reloc_pose", d_rvec);
  NEED("slam_reloc_pose", d_tvec);
  NEED("slam_reloc_pose", d_ninl);
  NEED("slam_reloc_pose", d_count);
  NEED("slam_reloc_pose", d_P);
  NEED("slam_reloc_pose", d_poses);
  NEED("slam_reloc_pose", d_count_out);
  SLAM_REQUIRE(d_poses != d_prior, "slam_reloc_pose: d_poses aliases d_prior");
  k_reloc_pose<<<nblk(batch, kWave), kWave, 0, slam::as_stream(stream)>>>(
      d_rvec, d_tvec, d_ninl, d_count, d_P, d_prior, batch, min_inliers, d_poses, d_count_out);
  SLAM_LAUNCHED("k_reloc_pose");
  return SLAM_OK;
}
