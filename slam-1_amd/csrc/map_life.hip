// Landmark life cycle of a device-resident map (include/slam355.h, "Landmark
// life cycle"): score, spawn, cull, compact.
//
//   k_map_score      one lane per landmark, a loop over the batch: consecutive
//                    lanes read consecutive uv / good, no atomics;
//   k_spawn_claim    one workgroup per frame: every eligible entry races its k
//                    into the claim word of its keypoint (workgroup-scope
//                    atomicMin, as k_unique), the winners are counted;
//   k_spawn_scatter  one workgroup per frame: sums the counts of the frames
//                    before its own, ranks its winners (wg_rank, wg_scan.hpp)
//                    and writes landmark, owner and track row;
//   k_map_cull       one lane per landmark;
//   k_compact_count / k_compact_scan / k_compact_scatter
//                    blocks of 1024 landmarks count their live ones, one
//                    workgroup scans the block counts, the blocks scatter;
//   k_rows_remap     one workgroup per frame: order-preserving compaction of
//                    the track rows through the remap table;
//   k_fuse_init / k_fuse_pairs / k_fuse_apply
//                    one rank key per landmark, one lane per (frame, landmark)
//                    that lost its keypoint: a 64-bit atomicMin of the better
//                    key into the worse landmark's word, then one lane per
//                    landmark walks the words to its root and merges;
//   k_rows_fuse      one workgroup per frame: the rows of one merged landmark
//                    race for its claim word, the winners are compacted.
// Nothing here waits for another workgroup: what one launch leaves for the
// next goes through memory and the launch boundary.
#include <climits>

#include "common.hpp"
#include "hamming_bits.hpp"
#include "wg_scan.hpp"

namespace {

constexpr int kScoreWG = 256;
constexpr int kItemWG = 1024;  // one workgroup per frame / per block of landmarks
constexpr int kWaves = kItemWG / kWave;

__global__ __launch_bounds__(kScoreWG) void k_map_score(
    const float* __restrict__ uv, const uint8_t* __restrict__ good,
    const int32_t* __restrict__ nq_arr, int x_cap, int batch, int frame0,
    int32_t* __restrict__ visible, int32_t* __restrict__ found, int32_t* __restrict__ last) {
  const int i = blockIdx.x * kScoreWG + threadIdx.x;
  if (i >= x_cap) return;
  int v = 0, f = 0, l = INT_MIN;
#pragma unroll 8
  for (int b = 0; b < batch; ++b) {
    const bool in = i < nq_arr[b];  // i < x_cap already; a negative nq admits nobody
    const size_t o = (size_t)b * x_cap + i;
    const float x = in ? uv[2 * o] : __builtin_nanf("");
    const uint8_t g = in ? good[o] : (uint8_t)0;
    v += isfinite(x) ? 1 : 0;
    if (g) {
      ++f;
      l = frame0 + b;
    }
  }
  if (v) visible[i] += v;
  if (f) {
    found[i] += f;
    last[i] = max(last[i], l);
  }
}

struct SpawnArgs {
  const double* Xc;
  const int2* pairs;
  const int32_t* count;
  const float* kp;
  const uint4* kp_desc;
  const int32_t* nkp;
  int32_t* owner;
  const double* poses;
  const uint8_t* spawn;
  double* X;
  uint4* desc;
  int32_t *visible, *found, *born, *last, *n;
  double* rows;
  int32_t *rows_count, *spawned, *dropped;
  int32_t* claim;  // workspace: [batch][kp_cap] claim words,
  int32_t* total;  //            [batch] candidates per frame,
  int32_t* n0;     //            the count on entry
  double z_min, z_max;
  int p_cap, kp_cap, x_cap, rows_cap, batch, frame0;
};

__global__ __launch_bounds__(kItemWG) void k_spawn_claim(const SpawnArgs a) {
  __shared__ int red[kWaves];
  const int b = blockIdx.x, t = threadIdx.x;
  if (b == 0 && t == 0) *a.n0 = clamp_count(*a.n, a.x_cap);
  if (!a.spawn[b]) {  // uniform
    if (t == 0) a.total[b] = 0;
    return;
  }
  const int count = clamp_count(a.count[b], a.p_cap), nkp = clamp_count(a.nkp[b], a.kp_cap);
  const double* Xc = a.Xc + (size_t)b * a.p_cap * 3;
  const int2* pairs = a.pairs + (size_t)b * a.p_cap;
  const int32_t* owner = a.owner + (size_t)b * a.kp_cap;
  int32_t* claim = a.claim + (size_t)b * a.kp_cap;
  for (int j = t; j < nkp; j += kItemWG)
    __hip_atomic_store(&claim[j], INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();
  for (int k = t; k < count; k += kItemWG) {
    const int j = pairs[k].x;
    if ((unsigned)j >= (unsigned)nkp || owner[j] != -1) continue;
    const double x = Xc[3 * (size_t)k], y = Xc[3 * (size_t)k + 1], z = Xc[3 * (size_t)k + 2];
    if (isfinite(x) && isfinite(y) && isfinite(z) && a.z_min < z && z < a.z_max)
      __hip_atomic_fetch_min(&claim[j], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  // a claim word equals k only if the eligible entry k put it there
  int c = 0;
  for (int k = t; k < count; k += kItemWG) {
    const int j = pairs[k].x;
    if ((unsigned)j < (unsigned)nkp &&
        __hip_atomic_load(&claim[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == k)
      ++c;
  }
  c = wg_sum<kItemWG>(c, red);
  if (t == 0) a.total[b] = c;
}

__global__ __launch_bounds__(kItemWG) void k_spawn_scatter(const SpawnArgs a) {
  __shared__ int red[kWaves];
  const int b = blockIdx.x, t = threadIdx.x;
  // batch <= kItemWG: one frame total per lane; p_cap <= 2^20 keeps the sums below 2^30
  const int mine = t < a.batch ? a.total[t] : 0;
  const int before = wg_sum<kItemWG>(t < b ? mine : 0, red);
  const int n0 = *a.n0;
  if (b == 0) {
    const int all = wg_sum<kItemWG>(mine, red);
    if (t == 0) {
      *a.n = min(n0 + all, a.x_cap);
      *a.dropped = max(n0 + all - a.x_cap, 0);
    }
  }
  const int room = max(a.x_cap - n0 - before, 0);  // landmarks this frame may still take
  if (!a.spawn[b]) {
    if (t == 0) a.spawned[b] = 0;
    return;
  }
  const int count = clamp_count(a.count[b], a.p_cap), nkp = clamp_count(a.nkp[b], a.kp_cap);
  const double* Xc = a.Xc + (size_t)b * a.p_cap * 3;
  const int2* pairs = a.pairs + (size_t)b * a.p_cap;
  const float* kp = a.kp + (size_t)b * a.kp_cap * 5;
  const uint4* kd = a.kp_desc + (size_t)b * a.kp_cap * 2;
  int32_t* owner = a.owner + (size_t)b * a.kp_cap;
  const int32_t* claim = a.claim + (size_t)b * a.kp_cap;
  double* rows = a.rows + (size_t)b * a.rows_cap * 4;
  const int rc0 = clamp_count(a.rows_count[b], a.rows_cap);
  const double* T = a.poses + 16 * (size_t)b;
  int carry = 0;  // candidates of this frame ranked so far (uniform)
  for (int base = 0; base < count; base += kItemWG) {
    const int k = base + t;
    int j = -1;
    if (k < count) j = pairs[k].x;
    const bool cand = (unsigned)j < (unsigned)nkp && claim[j] == k;
    int tot;
    const int r = carry + wg_rank<kItemWG>(cand, red, tot);
    carry += tot;
    if (!cand || r >= room) continue;
    const int i = n0 + before + r;  // < x_cap
    const double x = Xc[3 * (size_t)k], y = Xc[3 * (size_t)k + 1], z = Xc[3 * (size_t)k + 2];
#pragma unroll
    for (int c = 0; c < 3; ++c)
      a.X[3 * (size_t)i + c] = T[4 * c] * x + T[4 * c + 1] * y + T[4 * c + 2] * z + T[4 * c + 3];
    a.desc[2 * (size_t)i] = kd[2 * (size_t)j];
    a.desc[2 * (size_t)i + 1] = kd[2 * (size_t)j + 1];
    a.visible[i] = 1;
    a.found[i] = 1;
    a.born[i] = a.frame0 + b;
    a.last[i] = a.frame0 + b;
    owner[j] = i;
    const int row = rc0 + r;
    if (row < a.rows_cap) {
      double* o = rows + 4 * (size_t)row;
      o[0] = (double)(a.frame0 + b);
      o[1] = (double)i;
      o[2] = (double)kp[5 * (size_t)j];
      o[3] = (double)kp[5 * (size_t)j + 1];
    }
  }
  if (t == 0) {
    const int acc = min(carry, room);
    a.spawned[b] = acc;
    a.rows_count[b] = min(rc0 + acc, a.rows_cap);
  }
}

__global__ __launch_bounds__(kScoreWG) void k_map_cull(
    double* __restrict__ X, const int32_t* __restrict__ visible, const int32_t* __restrict__ found,
    const int32_t* __restrict__ born, const int32_t* __restrict__ n_ptr, int x_cap, int now,
    int min_visible, int ratio_num, int ratio_den, int age, int min_found,
    int32_t* __restrict__ nculled) {
  const int i = blockIdx.x * kScoreWG + threadIdx.x;
  if (i >= clamp_count(*n_ptr, x_cap)) return;
  if (X[3 * (size_t)i] != X[3 * (size_t)i]) return;  // dead already
  const long long v = visible[i], f = found[i];
  const bool weak = v >= min_visible && (long long)ratio_den * f < (long long)ratio_num * v;
  const bool stale = (long long)now - born[i] >= age && f < min_found;
  if (!(weak || stale)) return;
  const double nan = __builtin_nan("");
  X[3 * (size_t)i] = nan;
  X[3 * (size_t)i + 1] = nan;
  X[3 * (size_t)i + 2] = nan;
  atomicAdd(nculled, 1);  // one add per wave after the compiler's lane count
}

__device__ __forceinline__ bool alive(const double* X, int i, int n) {
  return i < n && X[3 * (size_t)i] == X[3 * (size_t)i];
}

// d_remap doubles as the scratch of the three launches: block blk keeps its
// count, then its base, in remap[blk * kItemWG] until its own scatter
// overwrites that word with the landmark's new index.
__global__ __launch_bounds__(kItemWG) void k_compact_count(const double* __restrict__ X,
                                                           const int32_t* __restrict__ n_ptr,
                                                           int x_cap, int32_t* __restrict__ remap) {
  __shared__ int red[kWaves];
  const int n = clamp_count(*n_ptr, x_cap);
  const int c = wg_sum<kItemWG>(alive(X, blockIdx.x * kItemWG + threadIdx.x, n) ? 1 : 0, red);
  if (threadIdx.x == 0) remap[(size_t)blockIdx.x * kItemWG] = c;
}

__global__ __launch_bounds__(kItemWG) void k_compact_scan(int nb, int32_t* __restrict__ remap,
                                                          int32_t* __restrict__ n_out) {
  __shared__ int wtot[kWaves];
  const int t = threadIdx.x;
  int carry = 0;  // live landmarks of the blocks scanned so far (uniform)
  for (int base = 0; base < nb; base += kItemWG) {
    const int blk = base + t;
    const int c = blk < nb ? remap[(size_t)blk * kItemWG] : 0;
    int tot;
    const int before = carry + wg_exscan<kItemWG>(c, wtot, tot);
    if (blk < nb) remap[(size_t)blk * kItemWG] = before;
    carry += tot;
  }
  if (t == 0) *n_out = carry;
}

struct CompactArgs {
  const double* X;
  const uint4* desc;
  const int32_t *visible, *found, *born, *last, *n;
  double* X_out;
  uint4* desc_out;
  int32_t *visible_out, *found_out, *born_out, *last_out, *remap;
  int x_cap;
};

__global__ __launch_bounds__(kItemWG) void k_compact_scatter(const CompactArgs a) {
  __shared__ int red[kWaves];
  __shared__ int base_s;
  const int i = blockIdx.x * kItemWG + threadIdx.x;
  const int n = clamp_count(*a.n, a.x_cap);
  if (threadIdx.x == 0) base_s = a.remap[(size_t)blockIdx.x * kItemWG];
  const bool keep = alive(a.X, i, n);
  int tot;
  const int r = wg_rank<kItemWG>(keep, red, tot);  // its barriers publish base_s as well
  if (i >= a.x_cap) return;
  const int d = base_s + r;
  a.remap[i] = keep ? d : -1;
  if (!keep) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) a.X_out[3 * (size_t)d + c] = a.X[3 * (size_t)i + c];
  a.desc_out[2 * (size_t)d] = a.desc[2 * (size_t)i];
  a.desc_out[2 * (size_t)d + 1] = a.desc[2 * (size_t)i + 1];
  a.visible_out[d] = a.visible[i];
  a.found_out[d] = a.found[i];
  a.born_out[d] = a.born[i];
  a.last_out[d] = a.last[i];
}

__global__ __launch_bounds__(kItemWG) void k_rows_remap(
    const double* __restrict__ rows, const int32_t* __restrict__ count_arr, int rows_cap,
    const int32_t* __restrict__ remap, int x_cap, double* __restrict__ rows_out,
    int32_t* __restrict__ count_out) {
  __shared__ int red[kWaves];
  const int b = blockIdx.x, t = threadIdx.x;
  const int count = clamp_count(count_arr[b], rows_cap);
  rows += (size_t)b * rows_cap * 4;
  rows_out += (size_t)b * rows_cap * 4;
  int carry = 0;
  for (int base = 0; base < count; base += kItemWG) {
    const int k = base + t;
    int l = -1;
    if (k < count) {
      const double v = rows[4 * (size_t)k + 1];
      if (v > -1.0 && v < (double)x_cap) l = remap[(int)v];
    }
    int tot;
    const int r = carry + wg_rank<kItemWG>(l >= 0, red, tot);
    carry += tot;
    if (l >= 0) {  // r <= k < rows_cap
      double* o = rows_out + 4 * (size_t)r;
      o[0] = rows[4 * (size_t)k];
      o[1] = (double)l;
      o[2] = rows[4 * (size_t)k + 2];
      o[3] = rows[4 * (size_t)k + 3];
    }
  }
  if (t == 0) count_out[b] = carry;
}

struct FuseArgs {
  const float* uv;
  const double* z;
  const int32_t* idx2;
  const uint8_t *good0, *good;
  const int32_t *owner, *nq;
  double* X;
  const uint4* desc;
  int32_t *visible, *found, *born, *last;
  const int32_t* n;
  int32_t *to, *nfused;
  unsigned long long* key;  // workspace: [x_cap] rank key of the best partner so far
  double px2, rel_depth;
  int max_dist, kp_cap, x_cap;
};

// lower key = better rank: more often found, then the lower index
__device__ __forceinline__ unsigned long long rank_key(const int32_t* found, int i) {
  return ((unsigned long long)(uint32_t)(INT_MAX - max(found[i], 0)) << 32) | (uint32_t)i;
}

__global__ __launch_bounds__(kScoreWG) void k_fuse_init(const FuseArgs a) {
  const int i = blockIdx.x * kScoreWG + threadIdx.x;
  if (i == 0) *a.nfused = 0;
  if (i < a.x_cap) a.key[i] = rank_key(a.found, i);
}

__global__ __launch_bounds__(kScoreWG) void k_fuse_pairs(const FuseArgs a) {
  const int l = blockIdx.x * kScoreWG + threadIdx.x, b = blockIdx.y;
  const int n = clamp_count(*a.n, a.x_cap);
  const int lim = min(clamp_count(a.nq[b], a.x_cap), n);  // l and w lie below nq_b and below *d_n
  if (l >= lim) return;
  const size_t o = (size_t)b * a.x_cap;
  if (!a.good0[o + l] || a.good[o + l]) return;  // passed the descriptor tests, lost the keypoint
  const int j = a.idx2[2 * (o + l)];
  if ((unsigned)j >= (unsigned)a.kp_cap) return;
  const int w = a.owner[(size_t)b * a.kp_cap + j];
  if ((unsigned)w >= (unsigned)lim || w == l) return;
  if (a.X[3 * (size_t)l] != a.X[3 * (size_t)l] || a.X[3 * (size_t)w] != a.X[3 * (size_t)w]) return;
  const float ul = a.uv[2 * (o + l)], vl = a.uv[2 * (o + l) + 1];
  const float uw = a.uv[2 * (o + w)], vw = a.uv[2 * (o + w) + 1];
  if (!(isfinite(ul) && isfinite(vl) && isfinite(uw) && isfinite(vw))) return;
  const double du = (double)ul - (double)uw, dv = (double)vl - (double)vw;
  if (!(du * du + dv * dv <= a.px2)) return;
  const double zl = a.z[o + l], zw = a.z[o + w];
  if (!(fabs(zl - zw) <= a.rel_depth * (zl < zw ? zl : zw))) return;  // NaN on either side: no pair
  const uint4 l0 = a.desc[2 * (size_t)l], l1 = a.desc[2 * (size_t)l + 1];
  const uint32_t dl[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
  if ((int)hd8(dl, a.desc[2 * (size_t)w], a.desc[2 * (size_t)w + 1]) > a.max_dist) return;
  const unsigned long long kl = rank_key(a.found, l), kw = rank_key(a.found, w);
  // kl != kw (the indices differ): the worse of the two learns of the better
  atomicMin(&a.key[kl < kw ? w : l], kl < kw ? kl : kw);
}

__global__ __launch_bounds__(kScoreWG) void k_fuse_apply(const FuseArgs a) {
  const int i = blockIdx.x * kScoreWG + threadIdx.x;
  if (i >= a.x_cap) return;
  int r = i;
  if (i < clamp_count(*a.n, a.x_cap)) {
    // the keys are read-only here; every hop strictly improves the rank
    for (int hop = 0; hop < a.x_cap; ++hop) {
      const int p = (int)(a.key[r] & 0xFFFFFFFFull);
      if (p == r || (unsigned)p >= (unsigned)a.x_cap) break;
      r = p;
    }
  }
  a.to[i] = r;
  if (r == i) return;
  // only roots receive, and a root is not fused: i's own counters are final
  atomicAdd(&a.visible[r], a.visible[i]);
  atomicAdd(&a.found[r], a.found[i]);
  atomicMin(&a.born[r], a.born[i]);
  atomicMax(&a.last[r], a.last[i]);
  const double nan = __builtin_nan("");
  a.X[3 * (size_t)i] = nan;
  a.X[3 * (size_t)i + 1] = nan;
  a.X[3 * (size_t)i + 2] = nan;
  atomicAdd(a.nfused, 1);  // one add per wave after the compiler's lane count
}

// The landmark that row k stands for after a fuse, or -1 for a row that is
// copied as it is; own: the row is the survivor's own observation.
__device__ __forceinline__ int fused_landmark(const double* rows, int k, const int32_t* to,
                                              int x_cap, bool& own) {
  own = false;
  const double v = rows[4 * (size_t)k + 1];
  if (!(v >= 0.0 && v < (double)x_cap)) return -1;
  const int l = (int)v;
  if ((double)l != v) return -1;
  const int r = to[l];
  if ((unsigned)r >= (unsigned)x_cap) return -1;
  own = r == l;
  return r;
}

__global__ __launch_bounds__(kItemWG) void k_rows_fuse(
    const double* __restrict__ rows, const int32_t* __restrict__ count_arr, int rows_cap,
    const int32_t* __restrict__ to, int x_cap, int32_t* claim, double* __restrict__ rows_out,
    int32_t* __restrict__ count_out) {
  __shared__ int red[kWaves];
  const int b = blockIdx.x, t = threadIdx.x;
  const int count = clamp_count(count_arr[b], rows_cap);
  rows += (size_t)b * rows_cap * 4;
  rows_out += (size_t)b * rows_cap * 4;
  claim += (size_t)b * x_cap;
  bool own;
  // every row sets the word it will race for: the workspace needs no memset
  for (int k = t; k < count; k += kItemWG) {
    const int r = fused_landmark(rows, k, to, x_cap, own);
    if (r >= 0) __hip_atomic_store(&claim[r], INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  // k < 65536: the survivor's own rows come before all others, then the lowest k
  for (int k = t; k < count; k += kItemWG) {
    const int r = fused_landmark(rows, k, to, x_cap, own);
    if (r >= 0)
      __hip_atomic_fetch_min(&claim[r], (own ? 0 : 65536) + k, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();
  int carry = 0;
  for (int base = 0; base < count; base += kItemWG) {
    const int k = base + t;
    int r = -1;
    bool keep = false;
    if (k < count) {
      r = fused_landmark(rows, k, to, x_cap, own);
      keep = r < 0 || __hip_atomic_load(&claim[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) ==
                          (own ? 0 : 65536) + k;
    }
    int tot;
    const int d = carry + wg_rank<kItemWG>(keep, red, tot);
    carry += tot;
    if (keep) {  // d <= k < rows_cap
      double* o = rows_out + 4 * (size_t)d;
      o[0] = rows[4 * (size_t)k];
      o[1] = r >= 0 ? (double)r : rows[4 * (size_t)k + 1];
      o[2] = rows[4 * (size_t)k + 2];
      o[3] = rows[4 * (size_t)k + 3];
    }
  }
  if (t == 0) count_out[b] = carry;
}

size_t spawn_ws_bytes(int batch, int kp_cap) {
  return ((size_t)batch * kp_cap + batch + 1) * sizeof(int32_t);
}

size_t fuse_ws_bytes(int x_cap) { return (size_t)x_cap * sizeof(unsigned long long); }

size_t rows_fuse_ws_bytes(int batch, int x_cap) { return (size_t)batch * x_cap * sizeof(int32_t); }

}  // namespace

extern "C" int slam_map_score(const float* d_uv, const uint8_t* d_good, const int32_t* d_nq,
                              int x_cap, int batch, int frame0, int32_t* d_visible,
                              int32_t* d_found, int32_t* d_last, void* stream) {
  SLAM_REQUIRE(x_cap >= 1 && x_cap <= kMaxLandmarks, "slam_map_score: x_cap %d not in 1..%d", x_cap,
               kMaxLandmarks);
  SLAM_REQUIRE(batch >= 1 && batch <= 65535, "slam_map_score: batch %d not in 1..65535", batch);
  NEED("slam_map_score", d_uv);
  NEED("slam_map_score", d_good);
  NEED("slam_map_score", d_nq);
  NEED("slam_map_score", d_visible);
  NEED("slam_map_score", d_found);
  NEED("slam_map_score", d_last);
  k_map_score<<<nblk(x_cap, kScoreWG), kScoreWG, 0, slam::as_stream(stream)>>>(
      d_uv, d_good, d_nq, x_cap, batch, frame0, d_visible, d_found, d_last);
  SLAM_LAUNCHED("k_map_score");
  return SLAM_OK;
}

extern "C" int slam_map_spawn_workspace_bytes(int batch, int kp_cap, size_t* bytes) {
  SLAM_REQUIRE(batch >= 1 && batch <= kItemWG, "slam_map_spawn_workspace_bytes: batch %d not in 1..%d",
               batch, kItemWG);
  SLAM_REQUIRE(kp_cap >= 1 && kp_cap <= 65535,
               "slam_map_spawn_workspace_bytes: kp_cap %d not in 1..65535", kp_cap);
  NEED("slam_map_spawn_workspace_bytes", bytes);
  *bytes = spawn_ws_bytes(batch, kp_cap);
  return SLAM_OK;
}

extern "C" int slam_map_spawn(const double* d_Xc, const int32_t* d_pairs, const int32_t* d_count,
                              int p_cap, const float* d_kp, const uint8_t* d_kp_desc,
                              const int32_t* d_nkp, int kp_cap, int32_t* d_owner,
                              const double* d_poses, const uint8_t* d_spawn, int batch,
                              double z_min, double z_max, int frame0, double* d_X, uint8_t* d_desc,
                              int32_t* d_visible, int32_t* d_found, int32_t* d_born,
                              int32_t* d_last, int32_t* d_n, int x_cap, double* d_rows,
                              int32_t* d_rows_count, int rows_cap, int32_t* d_spawned,
                              int32_t* d_dropped, void* d_ws, size_t ws_size, void* stream) {
  SLAM_REQUIRE(batch >= 1 && batch <= kItemWG, "slam_map_spawn: batch %d not in 1..%d", batch,
               kItemWG);
  SLAM_REQUIRE(p_cap >= 1 && p_cap <= (1 << 20), "slam_map_spawn: p_cap %d not in 1..1 << 20", p_cap);
  SLAM_REQUIRE(kp_cap >= 1 && kp_cap <= 65535, "slam_map_spawn: kp_cap %d not in 1..65535", kp_cap);
  SLAM_REQUIRE(x_cap >= 1 && x_cap <= kMaxLandmarks, "slam_map_spawn: x_cap %d not in 1..%d", x_cap,
               kMaxLandmarks);
  SLAM_REQUIRE(rows_cap >= (x_cap < kp_cap ? x_cap : kp_cap),
               "slam_map_spawn: rows_cap %d < min(x_cap %d, kp_cap %d)", rows_cap, x_cap, kp_cap);
  SLAM_REQUIRE(z_min < z_max, "slam_map_spawn: z_min %g < z_max %g does not hold", z_min, z_max);
  NEED("slam_map_spawn", d_Xc);
  NEED("slam_map_spawn", d_pairs);
  NEED("slam_map_spawn", d_count);
  NEED("slam_map_spawn", d_kp);
  NEED("slam_map_spawn", d_kp_desc);
  NEED("slam_map_spawn", d_nkp);
  NEED("slam_map_spawn", d_owner);
  NEED("slam_map_spawn", d_poses);
  NEED("slam_map_spawn", d_spawn);
  NEED("slam_map_spawn", d_X);
  NEED("slam_map_spawn", d_desc);
  NEED("slam_map_spawn", d_visible);
  NEED("slam_map_spawn", d_found);
  NEED("slam_map_spawn", d_born);
  NEED("slam_map_spawn", d_last);
  NEED("slam_map_spawn", d_n);
  NEED("slam_map_spawn", d_rows);
  NEED("slam_map_spawn", d_rows_count);
  NEED("slam_map_spawn", d_spawned);
  NEED("slam_map_spawn", d_dropped);
  NEED("slam_map_spawn", d_ws);
  NEED_ALIGNED16("slam_map_spawn", d_kp_desc);
  NEED_ALIGNED16("slam_map_spawn", d_desc);
  SLAM_REQUIRE(((uintptr_t)d_ws & 3) == 0, "slam_map_spawn: d_ws must be 4-byte aligned");
  if (ws_size < spawn_ws_bytes(batch, kp_cap)) {
    slam::set_error("slam_map_spawn: ws_size %zu < %zu", ws_size, spawn_ws_bytes(batch, kp_cap));
    return SLAM_ERR_WORKSPACE;
  }
  SpawnArgs a;
  a.Xc = d_Xc;
  a.pairs = reinterpret_cast<const int2*>(d_pairs);
  a.count = d_count;
  a.kp = d_kp;
  a.kp_desc = reinterpret_cast<const uint4*>(d_kp_desc);
  a.nkp = d_nkp;
  a.owner = d_owner;
  a.poses = d_poses;
  a.spawn = d_spawn;
  a.X = d_X;
  a.desc = reinterpret_cast<uint4*>(d_desc);
  a.visible = d_visible;
  a.found = d_found;
  a.born = d_born;
  a.last = d_last;
  a.n = d_n;
  a.rows = d_rows;
  a.rows_count = d_rows_count;
  a.spawned = d_spawned;
  a.dropped = d_dropped;
  a.claim = static_cast<int32_t*>(d_ws);
  a.total = a.claim + (size_t)batch * kp_cap;
  a.n0 = a.total + batch;
  a.z_min = z_min;
  a.z_max = z_max;
  a.p_cap = p_cap;
  a.kp_cap = kp_cap;
  a.x_cap = x_cap;
  a.rows_cap = rows_cap;
  a.batch = batch;
  a.frame0 = frame0;
  k_spawn_claim<<<batch, kItemWG, 0, slam::as_stream(stream)>>>(a);
  SLAM_LAUNCHED("k_spawn_claim");
  k_spawn_scatter<<<batch, kItemWG, 0, slam::as_stream(stream)>>>(a);
  SLAM_LAUNCHED("k_spawn_scatter");
  return SLAM_OK;
}

extern "C" int slam_map_cull(double* d_X, const int32_t* d_visible, const int32_t* d_found,
                             const int32_t* d_born, const int32_t* d_n, int x_cap, int now,
                             int min_visible, int ratio_num, int ratio_den, int age, int min_found,
                             int32_t* d_nculled, void* stream) {
  SLAM_REQUIRE(x_cap >= 1 && x_cap <= kMaxLandmarks, "slam_map_cull: x_cap %d not in 1..%d", x_cap,
               kMaxLandmarks);
  SLAM_REQUIRE(ratio_num >= 0 && ratio_den >= 1, "slam_map_cull: ratio %d / %d needs num >= 0, den >= 1",
               ratio_num, ratio_den);
  NEED("slam_map_cull", d_X);
  NEED("slam_map_cull", d_visible);
  NEED("slam_map_cull", d_found);
  NEED("slam_map_cull", d_born);
  NEED("slam_map_cull", d_n);
  NEED("slam_map_cull", d_nculled);
  SLAM_HIP(hipMemsetAsync(d_nculled, 0, sizeof(int32_t), slam::as_stream(stream)));
  k_map_cull<<<nblk(x_cap, kScoreWG), kScoreWG, 0, slam::as_stream(stream)>>>(
      d_X, d_visible, d_found, d_born, d_n, x_cap, now, min_visible, ratio_num, ratio_den, age,
      min_found, d_nculled);
  SLAM_LAUNCHED("k_map_cull");
  return SLAM_OK;
}

extern "C" int slam_map_compact(const double* d_X, const uint8_t* d_desc,
                                const int32_t* d_visible, const int32_t* d_found,
                                const int32_t* d_born, const int32_t* d_last, const int32_t* d_n,
                                int x_cap, double* d_X_out, uint8_t* d_desc_out,
                                int32_t* d_visible_out, int32_t* d_found_out, int32_t* d_born_out,
                                int32_t* d_last_out, int32_t* d_remap, int32_t* d_n_out,
                                void* stream) {
  SLAM_REQUIRE(x_cap >= 1 && x_cap <= kMaxLandmarks, "slam_map_compact: x_cap %d not in 1..%d", x_cap,
               kMaxLandmarks);
  NEED("slam_map_compact", d_X);
  NEED("slam_map_compact", d_desc);
  NEED("slam_map_compact", d_visible);
  NEED("slam_map_compact", d_found);
  NEED("slam_map_compact", d_born);
  NEED("slam_map_compact", d_last);
  NEED("slam_map_compact", d_n);
  NEED("slam_map_compact", d_X_out);
  NEED("slam_map_compact", d_desc_out);
  NEED("slam_map_compact", d_visible_out);
  NEED("slam_map_compact", d_found_out);
  NEED("slam_map_compact", d_born_out);
  NEED("slam_map_compact", d_last_out);
  NEED("slam_map_compact", d_remap);
  NEED("slam_map_compact", d_n_out);
  NEED_ALIGNED16("slam_map_compact", d_desc);
  NEED_ALIGNED16("slam_map_compact", d_desc_out);
  SLAM_REQUIRE(d_X_out != d_X && d_desc_out != d_desc && d_visible_out != d_visible &&
                   d_found_out != d_found && d_born_out != d_born && d_last_out != d_last,
               "slam_map_compact: an output aliases its input");
  SLAM_REQUIRE(d_n_out != d_n, "slam_map_compact: d_n_out aliases d_n");
  CompactArgs a;
  a.X = d_X;
  a.desc = reinterpret_cast<const uint4*>(d_desc);
  a.visible = d_visible;
  a.found = d_found;
  a.born = d_born;
  a.last = d_last;
  a.n = d_n;
  a.X_out = d_X_out;
  a.desc_out = reinterpret_cast<uint4*>(d_desc_out);
  a.visible_out = d_visible_out;
  a.found_out = d_found_out;
  a.born_out = d_born_out;
  a.last_out = d_last_out;
  a.remap = d_remap;
  a.x_cap = x_cap;
  const int nb = nblk(x_cap, kItemWG);
  hipStream_t s = slam::as_stream(stream);
  k_compact_count<<<nb, kItemWG, 0, s>>>(d_X, d_n, x_cap, d_remap);
  SLAM_LAUNCHED("k_compact_count");
  k_compact_scan<<<1, kItemWG, 0, s>>>(nb, d_remap, d_n_out);
  SLAM_LAUNCHED("k_compact_scan");
  k_compact_scatter<<<nb, kItemWG, 0, s>>>(a);
  SLAM_LAUNCHED("k_compact_scatter");
  return SLAM_OK;
}

extern "C" int slam_rows_remap(const double* d_rows, const int32_t* d_count, int rows_cap,
                               int batch, const int32_t* d_remap, int x_cap, double* d_rows_out,
                               int32_t* d_count_out, void* stream) {
  SLAM_REQUIRE(batch >= 1 && batch <= 65535, "slam_rows_remap: batch %d not in 1..65535", batch);
  SLAM_REQUIRE(rows_cap >= 1 && rows_cap <= 65535, "slam_rows_remap: rows_cap %d not in 1..65535",
               rows_cap);
  SLAM_REQUIRE(x_cap >= 1 && x_cap <= kMaxLandmarks, "slam_rows_remap: x_cap %d not in 1..%d", x_cap,
               kMaxLandmarks);
  NEED("slam_rows_remap", d_rows);
  NEED("slam_rows_remap", d_count);
  NEED("slam_rows_remap", d_remap);
  NEED("slam_rows_remap", d_rows_out);
  NEED("slam_rows_remap", d_count_out);
  SLAM_REQUIRE(d_rows_out != d_rows, "slam_rows_remap: d_rows_out aliases d_rows");
  k_rows_remap<<<batch, kItemWG, 0, slam::as_stream(stream)>>>(d_rows, d_count, rows_cap, d_remap,
                                                               x_cap, d_rows_out, d_count_out);
  SLAM_LAUNCHED("k_rows_remap");
  return SLAM_OK;
}

extern "C" int slam_map_fuse_workspace_bytes(int x_cap, size_t* bytes) {
  SLAM_REQUIRE(x_cap >= 1 && x_cap <= kMaxLandmarks,
               "slam_map_fuse_workspace_bytes: x_cap %d not in 1..%d", x_cap, kMaxLandmarks);
  NEED("slam_map_fuse_workspace_bytes", bytes);
  *bytes = fuse_ws_bytes(x_cap);
  return SLAM_OK;
}

extern "C" int slam_map_fuse(const float* d_uv, const double* d_z, const int32_t* d_idx2,
                             const uint8_t* d_good0, const uint8_t* d_good, const int32_t* d_owner,
                             const int32_t* d_nq, int batch, int kp_cap, double* d_X,
                             const uint8_t* d_desc, int32_t* d_visible, int32_t* d_found,
                             int32_t* d_born, int32_t* d_last, const int32_t* d_n, int x_cap,
                             double px, double rel_depth, int max_dist, int32_t* d_to,
                             int32_t* d_nfused, void* d_ws, size_t ws_size, void* stream) {
  SLAM_REQUIRE(batch >= 1 && batch <= 65535, "slam_map_fuse: batch %d not in 1..65535", batch);
  SLAM_REQUIRE(kp_cap >= 1 && kp_cap <= 65535, "slam_map_fuse: kp_cap %d not in 1..65535", kp_cap);
  SLAM_REQUIRE(x_cap >= 1 && x_cap <= kMaxLandmarks, "slam_map_fuse: x_cap %d not in 1..%d", x_cap,
               kMaxLandmarks);
  SLAM_REQUIRE(px > 0.0, "slam_map_fuse: px %g > 0 does not hold", px);
  SLAM_REQUIRE(rel_depth >= 0.0, "slam_map_fuse: rel_depth %g >= 0 does not hold", rel_depth);
  SLAM_REQUIRE(max_dist >= 0 && max_dist <= 256, "slam_map_fuse: max_dist %d not in 0..256", max_dist);
  NEED("slam_map_fuse", d_uv);
  NEED("slam_map_fuse", d_z);
  NEED("slam_map_fuse", d_idx2);
  NEED("slam_map_fuse", d_good0);
  NEED("slam_map_fuse", d_good);
  NEED("slam_map_fuse", d_owner);
  NEED("slam_map_fuse", d_nq);
  NEED("slam_map_fuse", d_X);
  NEED("slam_map_fuse", d_desc);
  NEED("slam_map_fuse", d_visible);
  NEED("slam_map_fuse", d_found);
  NEED("slam_map_fuse", d_born);
  NEED("slam_map_fuse", d_last);
  NEED("slam_map_fuse", d_n);
  NEED("slam_map_fuse", d_to);
  NEED("slam_map_fuse", d_nfused);
  NEED("slam_map_fuse", d_ws);
  NEED_ALIGNED16("slam_map_fuse", d_desc);
  SLAM_REQUIRE(((uintptr_t)d_ws & 7) == 0, "slam_map_fuse: d_ws must be 8-byte aligned");
  if (ws_size < fuse_ws_bytes(x_cap)) {
    slam::set_error("slam_map_fuse: ws_size %zu < %zu", ws_size, fuse_ws_bytes(x_cap));
    return SLAM_ERR_WORKSPACE;
  }
  FuseArgs a;
  a.uv = d_uv;
  a.z = d_z;
  a.idx2 = d_idx2;
  a.good0 = d_good0;
  a.good = d_good;
  a.owner = d_owner;
  a.nq = d_nq;
  a.X = d_X;
  a.desc = reinterpret_cast<const uint4*>(d_desc);
  a.visible = d_visible;
  a.found = d_found;
  a.born = d_born;
  a.last = d_last;
  a.n = d_n;
  a.to = d_to;
  a.nfused = d_nfused;
  a.key = static_cast<unsigned long long*>(d_ws);
  a.px2 = px * px;
  a.rel_depth = rel_depth;
  a.max_dist = max_dist;
  a.kp_cap = kp_cap;
  a.x_cap = x_cap;
  const int nb = nblk(x_cap, kScoreWG);
  hipStream_t s = slam::as_stream(stream);
  k_fuse_init<<<nb, kScoreWG, 0, s>>>(a);
  SLAM_LAUNCHED("k_fuse_init");
  k_fuse_pairs<<<dim3(nb, batch), kScoreWG, 0, s>>>(a);
  SLAM_LAUNCHED("k_fuse_pairs");
  k_fuse_apply<<<nb, kScoreWG, 0, s>>>(a);
  SLAM_LAUNCHED("k_fuse_apply");
  return SLAM_OK;
}

extern "C" int slam_rows_fuse_workspace_bytes(int batch, int x_cap, size_t* bytes) {
  SLAM_REQUIRE(batch >= 1 && batch <= 65535, "slam_rows_fuse_workspace_bytes: batch %d not in 1..65535",
               batch);
  SLAM_REQUIRE(x_cap >= 1 && x_cap <= kMaxLandmarks,
               "slam_rows_fuse_workspace_bytes: x_cap %d not in 1..%d", x_cap, kMaxLandmarks);
  NEED("slam_rows_fuse_workspace_bytes", bytes);
  *bytes = rows_fuse_ws_bytes(batch, x_cap);
  return SLAM_OK;
}

extern "C" int slam_rows_fuse(const double* d_rows, const int32_t* d_count, int rows_cap, int batch,
                              const int32_t* d_to, int x_cap, double* d_rows_out,
                              int32_t* d_count_out, void* d_ws, size_t ws_size, void* stream) {
  SLAM_REQUIRE(batch >= 1 && batch <= 65535, "slam_rows_fuse: batch %d not in 1..65535", batch);
  SLAM_REQUIRE(rows_cap >= 1 && rows_cap <= 65535, "slam_rows_fuse: rows_cap %d not in 1..65535",
               rows_cap);
  SLAM_REQUIRE(x_cap >= 1 && x_cap <= kMaxLandmarks, "slam_rows_fuse: x_cap %d not in 1..%d", x_cap,
               kMaxLandmarks);
  NEED("slam_rows_fuse", d_rows);
  NEED("slam_rows_fuse", d_count);
  NEED("slam_rows_fuse", d_to);
  NEED("slam_rows_fuse", d_rows_out);
  NEED("slam_rows_fuse", d_count_out);
  NEED("slam_rows_fuse", d_ws);
  SLAM_REQUIRE(d_rows_out != d_rows, "slam_rows_fuse: d_rows_out aliases d_rows");
  SLAM_REQUIRE(d_count_out != d_count, "slam_rows_fuse: d_count_out aliases d_count");
  SLAM_REQUIRE(((uintptr_t)d_ws & 3) == 0, "slam_rows_fuse: d_ws must be 4-byte aligned");
  if (ws_size < rows_fuse_ws_bytes(batch, x_cap)) {
    slam::set_error("slam_rows_fuse: ws_size %zu < %zu", ws_size, rows_fuse_ws_bytes(batch, x_cap));
    return SLAM_ERR_WORKSPACE;
  }
  k_rows_fuse<<<batch, kItemWG, 0, slam::as_stream(stream)>>>(
      d_rows, d_count, rows_cap, d_to, x_cap, static_cast<int32_t*>(d_ws), d_rows_out, d_count_out);
  SLAM_LAUNCHED("k_rows_fuse");
  return SLAM_OK;
}
