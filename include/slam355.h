/*
 * slam355.h — C ABI of libslam355.so, the MI355X (gfx950) hot path of the
 * DavidHan008/SLAM-1 stereo front end and local bundle adjustment.
 *
 * Conventions (every entry point):
 *   - Pointers named d_* are caller-owned DEVICE pointers (HBM).  Pointers named
 *     h_* are host pointers.  Nothing is allocated inside a hot call; scratch is
 *     a caller-provided workspace sized by the matching *_workspace_bytes query.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Every
 *     compute call is asynchronous on that stream.
 *   - Return value: 0 = ok; < 0 = error.  slam_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 *   - Ragged batches: per-item element counts live in DEVICE int32 arrays so a
 *     pipeline never has to synchronise to learn them; kernels clamp every
 *     count to the stated capacity.
 *
 * The reference (Python + OpenCV + scipy) has no FFI; each function below
 * replaces the Python/OpenCV call named in its comment, and the Python host
 * package `slam355` (slam-1_amd/slam355) keeps the reference's function names
 * and signatures on top of these calls.
 */
#ifndef SLAM355_H
#define SLAM355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM355_ABI_VERSION 1

/* Error codes. */
#define SLAM_OK 0
#define SLAM_ERR_ARG (-1)      /* invalid argument / shape                  */
#define SLAM_ERR_HIP (-2)      /* HIP runtime error (launch, device)        */
#define SLAM_ERR_WORKSPACE (-3) /* workspace too small                      */
#define SLAM_ERR_COMM (-4)     /* collective error                          */

int slam_abi_version(void);
const char* slam_last_error(void);
/* Number of visible devices (0 when no GPU); never fails. */
int slam_device_count(void);

/* ------------------------------------------------------------------------
 * Brute-force Hamming kNN-2 + Lowe ratio test.
 *
 * Replaces cv2.FlannBasedMatcher(LSH).knnMatch(des_q, des_t, k=2) followed by
 * the `m.distance < 0.7 * n.distance` loop:
 *   /root/reference/keypoint.py:40-51   (track_keypoints_left_to_right_new)
 *   /root/reference/Point3D.py:35-49  (find_2D_and_3D_correspondenses)
 *   /root/reference/tracking.py:14-30 (get_matches)
 * Exact search (FLANN-LSH is approximate).  Ties are broken by
 * the lower train index, as cv::BFMatcher does.
 *
 * Batch of `batch` independent (query set, train set) pairs.
 *   d_q    [batch][q_cap][32] u8     d_nq [batch] i32 (clamped to q_cap)
 *   d_t    [batch][t_cap][32] u8     d_nt [batch] i32 (clamped to t_cap)
 * Outputs for every valid query row (rows >= nq are not written):
 *   d_idx2  [batch][q_cap][2] i32  best / second-best train index (-1 = none)
 *   d_dist2 [batch][q_cap][2] i32  their Hamming distances      (-1 = none)
 *   d_good  [batch][q_cap]    u8   1 iff both exist and 10*d1 < 7*d2
 * (`10*d1 < 7*d2` == `d1 < 0.7*d2` for every integer d1, d2 in [0, 256].)
 * A train set with fewer than 2 rows yields no good matches, mirroring the
 * reference's ValueError truncation (keypoint.py:46-51).
 * t_cap must be <= 65535.  t_cap <= 16383 runs on the fp4 matrix cores
 * (knn2_mx_kernel: exact integer keys in f32), larger train sets on the
 * integer VALU (knn2_kernel); both give identical outputs.
 * ---------------------------------------------------------------------- */
int slam_hamming_knn2(const uint8_t* d_q, const int32_t* d_nq, int q_cap,
                      const uint8_t* d_t, const int32_t* d_nt, int t_cap,
                      int batch, int32_t* d_idx2, int32_t* d_dist2,
                      uint8_t* d_good, void* stream);

/* Kernel selection of slam_hamming_knn2 for A/B tests and benchmarks:
 * valu != 0 forces the integer-VALU kernel, 0 (default) the matrix-core one
 * where t_cap allows.  Process-wide; returns the previous setting. */
int slam_hamming_force_valu(int valu);

/* Order-preserving compaction of the good matches of slam_hamming_knn2:
 * d_pairs [batch][q_cap][2] i32 = (queryIdx, trainIdx) of the good rows in
 * query order (the `good` list of keypoint.py:47-49), d_count [batch] i32.
 * Optional extra gate (Point3D.py:45-46): if d_gate_xyz != NULL, a good
 * row q is kept only if |X[q][k]| < gate for k = 0,1,2, where
 * d_gate_xyz [batch][q_cap][3] f64. */
int slam_compact_matches(const int32_t* d_idx2, const uint8_t* d_good,
                         const int32_t* d_nq, int q_cap, int batch,
                         const double* d_gate_xyz, double gate,
                         int32_t* d_pairs, int32_t* d_count, void* stream);


/* ------------------------------------------------------------------------
 * Geometry of one tracking step (main.py:82-97), batched over frame pairs.
 * ---------------------------------------------------------------------- */

/* Gather of matched keypoints (keypoint.py:53-57, Point3D.py:50-52):
 * for k < count[b], (qi, ti) = pairs[b][k]:
 *   ptq[b][k] = (double)kpq[b][qi].xy, ptt[b][k] = (double)kpt[b][ti].xy,
 *   dq[b][k] = desq[b][qi], dt[b][k] = dest[b][ti]  (descriptors optional: NULL).
 * kp arrays are [batch][cap][5] f32 as written by slam_orb_tiles. */
int slam_gather_matches(const float* d_kpq, int kq_cap, const float* d_kpt, int kt_cap,
                        const uint8_t* d_desq, const uint8_t* d_dest, const int32_t* d_pairs,
                        const int32_t* d_count, int p_cap, int batch, double* d_ptq,
                        double* d_ptt, uint8_t* d_dq, uint8_t* d_dt, void* stream);

/* 2D-3D correspondences of find_2D_and_3D_correspondenses (Point3D.py:50-52):
 * for k < count[b], (qi, ti) = pairs[b][k]: Q1[b][k] = X[b][qi], q1[b][k] =
 * ptl[b][qi], q2[b][k] = (double)kp_next[b][ti].xy.  X [batch][xcap][3],
 * ptl [batch][xcap][2] f64; kp_next [batch][kcap][5] f32. */
int slam_gather_temporal(const double* d_X, const double* d_ptl, int xcap, const float* d_kp_next,
                         int kcap, const int32_t* d_pairs, const int32_t* d_count, int pcap,
                         int batch, double* d_Q1, double* d_q2, double* d_q1, void* stream);

/* cv2.findFundamentalMat(pts_left, pts_right, FM_LMEDS) mask (keypoint.py:59-66),
 * deterministic LMedS restated in oracle/fundamental.c: n_hyp seeded 7-point
 * hypotheses (300 = OpenCV's LMeDS count at confidence 0.99), min median of
 * the symmetric epipolar error, inliers err <= sigma^2 with OpenCV's robust
 * sigma.  d_m1/d_m2 [batch][cap][2] f64; d_mask [batch][cap] u8; d_F
 * [batch][9] (unit Frobenius norm); d_ninliers [batch] (-1: < 8 points / no model). */
int slam_fundamental_lmeds(const double* d_m1, const double* d_m2, const int32_t* d_count,
                           int cap, int batch, uint64_t seed, int item0, int n_hyp,
                           uint8_t* d_mask, double* d_F, int32_t* d_ninliers, void* stream);
/* slam_fundamental_lmeds on a caller-owned workspace d_ws of ws_len doubles (the
 * hypotheses' candidate matrices, written by one kernel and scored by the
 * next): the form for a hot loop.  Same results bit for bit.  A ws_len below
 * slam_fundamental_workspace_len(batch, n_hyp) returns SLAM_ERR_ARG with a
 * message naming the needed length, before any GPU call.  The workspace is the
 * caller's: calls that may overlap (other streams) need their own; it need not
 * be cleared between calls.  slam_fundamental_lmeds itself takes its workspace
 * from the stream's memory pool (hipMallocAsync / hipFreeAsync on `stream`). */
int slam_fundamental_lmeds_ws(const double* d_m1, const double* d_m2, const int32_t* d_count,
                              int cap, int batch, uint64_t seed, int item0, int n_hyp,
                              uint8_t* d_mask, double* d_F, int32_t* d_ninliers, double* d_ws,
                              long long ws_len, void* stream);
/* Doubles of slam_fundamental_lmeds_ws's workspace (28 per pair and hypothesis);
 * monotone in both arguments, 0 when either is <= 0. */
long long slam_fundamental_workspace_len(int batch, int n_hyp);

/* Order-preserving compaction of pairs[b][k] (k < count[b]) where mask[b][k] != 0
 * (the `pts_left[mask]` of keypoint.py:63-66). d_out must not alias d_pairs. */
int slam_filter_pairs(const int32_t* d_pairs, const int32_t* d_count, const uint8_t* d_mask,
                      int cap, int batch, int32_t* d_out, int32_t* d_out_count, void* stream);

/* cv2.triangulatePoints + dehomogenisation (Point3D.py:14-19): per point the
 * null vector of the 4x4 DLT system (rows x*P[2]-P[0], y*P[2]-P[1] of both
 * views), one-sided Jacobi SVD in f64.  d_ptl/d_ptr [batch][cap][2] f64,
 * d_X [batch][cap][3] f64.  P matrices are 3x4 row-major f64: shared by all
 * items (proj_stride 0) or one per item (proj_stride 12). */
int slam_triangulate(const double* d_ptl, const double* d_ptr, const int32_t* d_count, int cap,
                     int batch, const double* d_Pl, const double* d_Pr, int proj_stride,
                     double* d_X, void* stream);

/* cv2.solvePnPRansac(Q, q, K, zeros(5)) (transformation.py:11-13), restated
 * deterministically (oracle/geometry.c): n_hyp hypotheses of 5 points drawn
 * from splitmix64(seed, item0 + b, h), LM from r = t = 0 (hyp_iters), score =
 * #(|reprojection error| <= reproj_thresh), best = max score / lowest h, LM
 * refinement over its inliers (refine_iters).  One workgroup per item.
 * Outputs: d_rvec/d_tvec [batch][3] (X_cam = R(rvec) X + tvec), d_ninliers
 * [batch] (-1 when count < 5, the reference's `len(Q) > 4` guard, main.py:94),
 * d_mask [batch][cap] u8 inliers of the chosen hypothesis. */
int slam_pnp_ransac(const double* d_Q, const double* d_q, const int32_t* d_count, int cap,
                    int batch, const double* d_K, uint64_t seed, int item0, int n_hyp,
                    double reproj_thresh, int hyp_iters, int refine_iters, double* d_rvec,
                    double* d_tvec, int32_t* d_ninliers, uint8_t* d_mask, double* d_ws,
                    long long ws_len, void* stream);
/* Doubles of slam_pnp_ransac's workspace d_ws (the hypothesis poses); a d_ws of
 * fewer than this many doubles (ws_len) returns SLAM_ERR_WORKSPACE.  The
 * workspace is the caller's: calls that may overlap (other streams) need their own. */
long long slam_pnp_workspace_len(int batch, int n_hyp);
/* slam_pnp_ransac with a caller-owned EPnP scratch d_scratch of scratch_len
 * doubles (what the eigen kernel of a hypothesis hands to its beta kernel): the
 * form for a hot loop.  Same results bit for bit.  A scratch_len below
 * slam_pnp_scratch_len(batch, n_hyp) returns SLAM_ERR_WORKSPACE with a message
 * naming the needed length, before any GPU call.  The scratch is the caller's:
 * calls that may overlap (other streams) need their own; it need not be cleared
 * between calls.  slam_pnp_ransac itself takes its scratch from the stream's
 * memory pool (hipMallocAsync / hipFreeAsync on `stream`). */
int slam_pnp_ransac_ws(const double* d_Q, const double* d_q, const int32_t* d_count, int cap,
                       int batch, const double* d_K, uint64_t seed, int item0, int n_hyp,
                       double reproj_thresh, int hyp_iters, int refine_iters, double* d_rvec,
                       double* d_tvec, int32_t* d_ninliers, uint8_t* d_mask, double* d_ws,
                       long long ws_len, double* d_scratch, long long scratch_len, void* stream);
/* Doubles of slam_pnp_ransac_ws's scratch (106 per item and hypothesis);
 * monotone in both arguments, 0 when either is <= 0. */
long long slam_pnp_scratch_len(int batch, int n_hyp);

/* Pose chain of main.py:94-98, 120-124 (pose_{b+1} = pose_b @ T_b with
 * T_b = [Rodrigues(-rvec_b) | -tvec_b], transformation.py:15-19; when
 * d_ninliers[b] < 0 -- PnP skipped, main.py:94 -- the previous T is reused).
 * d_state [32] f64 = (pose, T) 4x4 row-major, read and updated in place so
 * consecutive batches chain on the device; d_poses [batch][16] f64 out.
 * Replaces the host loop slam355.pipeline.chain_poses. */
int slam_pose_chain(const double* d_rvec, const double* d_tvec, const int32_t* d_ninliers,
                    int batch, double* d_state, double* d_poses, void* stream);

/* The reference's stereo visual-odometry pose estimator
 * (visual_odometry.py:135-157 estimate_pose over the residuals of :65-81),
 * restated deterministically (oracle/vo.c): dof = (rotvec, t), T = [R | t];
 * residuals f (4N) = [proj(P T, Q2) - q1 (x row, y row), proj(P T^-1, Q1) - q2
 * (x row, y row)]; max_iter hypotheses of 6 points drawn WITH replacement from
 * splitmix64(seed, item0 + b, h) (np.random.choice(range(n), 6), :139), LM from
 * dof = 0 (lm_iters; least_squares(method='lm') at :142), error = sum over k of
 * |(f[2k], f[2k+1])| (the reshape((2N, 2)) of :144-146), sequential early stop
 * after early_stop non-improving hypotheses (:147-154; 5 in the reference).
 * One workgroup per item, one lane per hypothesis (max_iter <= 128).
 * d_q1/d_q2 [batch][cap][2], d_Q1/d_Q2 [batch][cap][3] f64, d_P 3x4 row-major.
 * Outputs: d_pose [batch][6] (rotvec, t) of the selected hypothesis (zeros when
 * none improved), d_best [batch] its index (-1 if none), d_ntried [batch]
 * hypotheses the sequential loop evaluates, d_err [batch] its error. */
int slam_vo_estimate_pose(const double* d_q1, const double* d_q2, const double* d_Q1,
                          const double* d_Q2, const int32_t* d_count, int cap, int batch,
                          const double* d_P, uint64_t seed, int item0, int max_iter,
                          int lm_iters, int early_stop, double* d_pose, int32_t* d_best,
                          int32_t* d_ntried, double* d_err, void* d_ws, size_t ws_bytes,
                          void* stream);
/* Workspace of slam_vo_estimate_pose: every hypothesis' dof and error
 * (the error is np.sum's order over the pair norms: 8192-chunks of pairwise sums). */
int slam_vo_pose_workspace_bytes(int batch, int max_iter, size_t* bytes);

/* reprojection_residuals(dof, q1, q2, Q1, Q2) (visual_odometry.py:65-81) for
 * one dof per item: d_dof [batch][6]; d_res [batch][4 * cap], the first
 * 4 * count[b] entries in the reference's flattened order. */
int slam_vo_residuals(const double* d_dof, const double* d_q1, const double* d_q2,
                      const double* d_Q1, const double* d_Q2, const int32_t* d_count, int cap,
                      int batch, const double* d_P, double* d_res, void* stream);

/* relative_to_abs3DPoints (Point3D.py:22-30) for a tracking batch:
 * d_abs[b][i] = (pose_b [X;1])[:3] / (pose_b [X;1])[3] for i < d_count[b];
 * d_rel, d_abs [batch][cap][3] f64, d_poses [batch][16] f64 row-major. */
int slam_rel_to_abs(const double* d_rel, const int32_t* d_count, int cap, int batch,
                    const double* d_poses, double* d_abs, void* stream);

/* ------------------------------------------------------------------------
 * Map association: appendKeyPoints (keypoint.py:101-122).
 *
 * For each of the N new absolute points (d_abs [N][3] f64, camera-frame
 * d_rel [N][3], image coordinates d_pts2d [N][2]) the exact nearest map point
 * (the reference's KDTree(Qs).query(k=1); squared distance summed x, y, z in
 * f64, ties -> lowest index) is taken as the landmark when its distance is
 * below threshold * |rel| (:113-115); otherwise the point is appended to the
 * map with the next index (:117-118).  Queries use the map as it was before
 * the call (the tree is built first, :109).  d_map [map_cap][3] f64 and the map
 * size d_M (device int32, updated in place: sequences of frames need no host
 * synchronisation).  M_bound is any host-side upper bound of *d_M (grid
 * sizing); M_bound + N <= map_cap is required.  d_n (nullable): device count
 * of valid points (<= N).  d_rows [N][4] f64 = [frame_index, landmark index,
 * u, v] (the reference's full_index_array rows).  Workspace from
 * slam_map_workspace_bytes(N, M_bound or map_cap). */
int slam_map_workspace_bytes(int max_queries, int map_cap, size_t* bytes);
int slam_map_associate(double* d_map, int32_t* d_M, int map_cap, int M_bound,
                       const double* d_abs, const double* d_rel, const double* d_pts2d,
                       const int32_t* d_n, int N, double threshold, int frame_index,
                       double* d_rows, void* d_ws, size_t ws_size, void* stream);
/* The local maps of a tracked batch's windows (main.py:120-127 per window of n
 * consecutive frame pairs; bench.py's tracked leg): for window w < n_win, map
 * d_maps[w] ([map_cap][3], map_cap >= n * cap) restarted empty (d_M[w] = 0)
 * and fed pairs b = w n + j, j < n, in order -- slam_map_associate of
 * d_abs[b], d_rel[b] ([cap][3]), d_pts2d[b] ([cap][2]), d_count[b] valid
 * points, frame_index j, rows into d_rows[b] ([cap][4]).  One call for the
 * whole batch, the same results as n_win * n slam_map_associate calls: pair j
 * of every window runs in one launch pair (2n launches instead of 2 n n_win);
 * workspace n_win * slam_map_workspace_bytes(cap, (n - 1) * cap). */
int slam_map_windows(double* d_maps, int32_t* d_M, int map_cap, int n_win, int n,
                     const double* d_abs, const double* d_rel, const double* d_pts2d,
                     const int32_t* d_count, int cap, double threshold, double* d_rows,
                     void* d_ws, size_t ws_size, void* stream);

/* ------------------------------------------------------------------------
 * Guided matching (search by projection): landmarks with descriptors are
 * projected into a frame with its predicted pose, each is compared only with
 * the keypoints inside a window round its predicted pixel, every keypoint goes
 * to at most one landmark, and the matches come out as track rows.  Five
 * steps, each asynchronous on `stream`, none allocating or synchronising.
 *
 * 1. Projection.  d_X [x_items][x_cap][3] f64 world points, x_items = batch, or
 *    1 when x_shared != 0 (one map, many frames); d_nx [batch] i32 (clamped to
 *    [0, x_cap]); d_poses [batch][16] f64 row-major camera-to-world, rigid (the
 *    d_poses of slam_rel_to_abs; R = its 3x3, t = its last column); d_P [12]
 *    f64, a 3x4 projection; margin >= 0.  In this order, without contraction:
 *      d    = X - t
 *      xc_k = R[0][k] d0 + R[1][k] d1 + R[2][k] d2          (R^T d, left to right)
 *      h_i  = P[i][0] xc0 + P[i][1] xc1 + P[i][2] xc2 + P[i][3]
 *      u = h0 / h2, v = h1 / h2
 *    valid iff xc2 > min_depth, h2 > 0, margin <= u < W - margin and
 *    margin <= v < H - margin.  d_uv [batch][x_cap][2] f32 = (float)u, (float)v,
 *    both NaN when invalid; d_z [batch][x_cap] f64 = xc2 (may be NULL).  Rows
 *    >= nx are not written.  batch <= 65535 (here and in step 3). */
int slam_project_landmarks(const double* d_X, int x_shared, const int32_t* d_nx, int x_cap,
                           int batch, const double* d_poses, const double* d_P, int W, int H,
                           double margin, double min_depth, float* d_uv, double* d_z,
                           void* stream);

/* 2. Cell index of a batch of keypoint sets.  d_kp [batch][kp_cap][5] f32 (the
 *    layout slam_orb_tiles writes: x, y first), d_nkp [batch] i32 (negative --
 *    ORB's overflow code -- counts as 0, otherwise clamped to kp_cap);
 *    cell in {16, 32, 64}; gw = ceil(W / cell), gh = ceil(H / cell), gw gh <=
 *    16384; kp_cap <= 65535.  A keypoint with 0 <= x < W and 0 <= y < H goes to
 *    cell (int)(y / cell) gw + (int)(x / cell); any other (NaN included) is left
 *    out.  d_cell_ptr [batch][gw gh + 1] i32: CSR offsets in row-major cell
 *    order; d_cell_kp [batch][kp_cap] i32: keypoint indices grouped by cell (the
 *    order inside a cell is unspecified; entries past the total are not
 *    written). */
int slam_kp_grid(const float* d_kp, const int32_t* d_nkp, int kp_cap, int batch, int W, int H,
                 int cell, int32_t* d_cell_ptr, int32_t* d_cell_kp, void* stream);

/* 3. Windowed Hamming kNN-2.  Queries: d_q [q_items][q_cap][32] u8 (q_items =
 *    batch, or 1 when q_shared != 0), d_quv [batch][q_cap][2] f32 window centre,
 *    d_qr [batch][q_cap] f32 window half-size, d_nq [batch].  Targets: d_t
 *    [batch][t_cap][32] u8, d_kp [batch][t_cap][5] f32, d_nt [batch] and the
 *    index of step 2 built from the same d_kp with the same W, H, cell.
 *    The result does not depend on the cell size.  For query i with finite u,
 *    v and r > 0, keypoint j < nt inside the image (0 <= kx < W, 0 <= ky < H:
 *    the keypoints step 2 indexes) is a candidate iff
 *      fabsf(kx_j - u) <= r && fabsf(ky_j - v) <= r        (f32, edge included)
 *    and the two smallest keys dist << 16 | j over the candidates are reported
 *    (ties to the lower index, as slam_hamming_knn2):
 *      d_idx2, d_dist2 [batch][q_cap][2] i32 (-1 = none)
 *      d_good [batch][q_cap] u8 = 1 iff d1 exists, d1 <= max_dist and either
 *             no second candidate exists or ratio_den d1 < ratio_num d2.
 *    Unlike slam_hamming_knn2, ONE candidate is enough for a good match: a
 *    single keypoint in a small window is the normal case, not a truncated
 *    search.  A query with non-finite uv or r <= 0 gets -1 / -1 / 0; rows >= nq
 *    are not written.  max_dist in 0..256, 0 < ratio_num <= ratio_den,
 *    t_cap <= 65535, q_cap <= 1 << 20; descriptors 16-byte aligned. */
int slam_hamming_window_knn2(const uint8_t* d_q, int q_shared, const float* d_quv,
                             const float* d_qr, const int32_t* d_nq, int q_cap,
                             const uint8_t* d_t, const float* d_kp, const int32_t* d_nt,
                             int t_cap, const int32_t* d_cell_ptr, const int32_t* d_cell_kp,
                             int W, int H, int cell, int batch, int max_dist, int ratio_num,
                             int ratio_den, int32_t* d_idx2, int32_t* d_dist2, uint8_t* d_good,
                             void* stream);

/* 4. One landmark per keypoint.  A keypoint that is the best match (d_idx2[.][0])
 *    of several good queries goes to the one with the smallest (d1, query
 *    index): an integer atomicMin of d1 << 22 | query, so the result does not
 *    depend on the order of arrival.  d_owner [batch][t_cap] i32 = the winning
 *    query or -1; d_good_out [batch][q_cap] u8 = d_good with the losers cleared
 *    (rows >= nq are not written; it may not alias d_good). */
int slam_match_unique(const int32_t* d_idx2, const int32_t* d_dist2, const uint8_t* d_good,
                      const int32_t* d_nq, int q_cap, int t_cap, int batch, int32_t* d_owner,
                      uint8_t* d_good_out, void* stream);

/* 5. Track rows.  d_rows [batch][rows_cap][4] f64 = [frame0 + b, landmark
 *    index, (double)kx, (double)ky] for the good queries of step 4 in ascending
 *    landmark order -- the row format of slam_map_associate -- and d_count
 *    [batch] i32.  rows_cap >= min(q_cap, kp_cap) (after step 4 every keypoint
 *    appears at most once); a smaller cap is an argument error. */
int slam_track_rows(const int32_t* d_idx2, const uint8_t* d_good, const int32_t* d_nq, int q_cap,
                    const float* d_kp, int kp_cap, int batch, int frame0, int rows_cap,
                    double* d_rows, int32_t* d_count, void* stream);

/* ------------------------------------------------------------------------
 * Robust pose refinement from track rows (motion-only bundle adjustment, the
 * pose optimisation that follows search by projection): start at the
 * predicted pose, minimise the robust reprojection error of the matched
 * landmarks, drop the matches that do not fit, repeat, and return the pose
 * with its information matrix.  Batched, asynchronous on `stream`; no
 * allocation, no workspace, no host synchronisation.
 *
 * Inputs.  d_rows [batch][rows_cap][4] f64 and d_count [batch] i32 (clamped to
 * [0, rows_cap]) as slam_track_rows writes them (frame, landmark, x, y; the
 * frame column is not read); d_X [n_x][3] f64 the map; d_poses [batch][16] f64
 * row-major camera-to-world as in slam_project_landmarks; d_P [12] f64 a 3x4
 * projection whose fourth column may be non-zero.
 *
 * Frame.  R, t from the input pose.  Observation k < count has landmark l and
 * pixel (x, y); with l outside [0, n_x) (NaN included) it is never valid.
 * Q_k = R^T (X_l - t) in the operation order of slam_project_landmarks.
 *
 * Parameters.  A left increment p = (w, v), starting at 0:
 *   X_cam = Rod(w) Q_k + v          (Rod: cv::Rodrigues; identity below |w| = 2^-52)
 *   h     = P[:, :3] X_cam + P[:, 3]
 *   r     = (h0 (1 / h2) - x, h1 (1 / h2) - y)
 * and the observation is VALID AT p iff X_cam[2] > min_depth and h2 > 0.  No
 * matrix logarithm is taken anywhere: an input pose with a rotation near pi is
 * as good as any other.  The 2x6 Jacobian is d(u, v)/dX_cam (for the general
 * P: ((P[0,:3] - u P[2,:3]) / h2, (P[1,:3] - v P[2,:3]) / h2)) times
 * [d(Rod(w) Q)/dw | I], the rotation block in the Gallego-Yezzi form
 * -R [Q]x (w w^T + (R^T - I) [w]x) / |w|^2, and -[R Q]x when |w|^2 < 1e-24.
 *
 * One round, over a fixed active set A: `iters` Levenberg-Marquardt iterations
 * with lambda starting at 1e-3.  H = sum J^T J, g = sum J^T r, cost = sum term
 * over A, where for loss 0 (linear) term = |r|^2, and for loss 1 huber,
 * 2 soft_l1, 3 cauchy (delta = loss_scale; the losses of slam_ba_problem) r and
 * J are scaled by sqrt(rho'(z)), z = |r|^2 / delta^2, and term = delta^2 rho(z).
 * The step solves (H + lambda max(diag H, 1e-12)) d = -g by Cholesky; the
 * trial p + d is accepted iff the factorisation succeeded, every observation
 * of A is valid at the trial and cost_trial < cost; lambda <- max(lambda / 10,
 * 1e-12) on accept, min(10 lambda, 1e12) on reject.
 *
 * Rounds.  A_0 = the observations valid at p = 0.  After each of the n_rounds
 * rounds EVERY observation is classified, not only those of A: it is an
 * inlier iff it is valid at p and its unweighted |r|^2 <= gate^2, and the next
 * round's A is the inliers -- an observation rejected in one round can come
 * back in the next.  Fewer than min_inliers inliers after a round: status 2.
 *
 * Outputs (d_poses_out may not alias d_poses).
 *   d_poses_out [batch][16]  R' = R Rod(w)^T, t' = t - R' v, last row 0 0 0 1
 *   d_mask [batch][rows_cap] u8  the last classification made (status 1: the
 *                            observations valid at the input pose); entries
 *                            >= count are not written
 *   d_ninl [batch] i32       the number of ones in it
 *   d_cost [batch] f64       sum of term over the final inliers at the final pose
 *   d_info [batch][36] f64   row-major, symmetric bit for bit: sum J~^T J~ over
 *                            the final inliers relinearised at the returned
 *                            pose (p = 0, Q <- X_cam, hence the -[X_cam]x
 *                            branch), J~ robust-weighted: the information of the
 *                            perturbation X_cam <- Exp(dw) X_cam + dv in the
 *                            order (dw, dv)
 *   d_status [batch] i32     0 ok; 1 fewer than min_inliers observations valid
 *                            at the input pose (nothing is optimised); 2 the
 *                            inliers fell below min_inliers after a round.
 * For status 1 and 2 d_poses_out is the input pose bit for bit, d_info and
 * d_cost are zeros and d_ninl is -1.
 *
 * Sums are formed per lane, per wave and then in wave order, so results equal
 * a sequential evaluation up to the rounding of the summation order only.
 * SLAM_ERR_ARG before any GPU call: a null pointer; batch or rows_cap outside
 * 1..65535; n_x < 0; n_rounds outside 1..8; iters outside 1..50; min_inliers
 * < 3; loss outside 0..3; loss_scale <= 0 with loss != 0; gate <= 0;
 * min_depth NaN. */
int slam_pose_refine(const double* d_rows, const int32_t* d_count, int rows_cap, int batch,
                     const double* d_X, int n_x, const double* d_poses, const double* d_P,
                     int loss, double loss_scale, double gate, double min_depth,
                     int n_rounds, int iters, int min_inliers,
                     double* d_poses_out, uint8_t* d_mask, int32_t* d_ninl, int32_t* d_status,
                     double* d_info, double* d_cost, void* stream);

/* ------------------------------------------------------------------------
 * Landmark life cycle: what a map does after a batch of frames was tracked --
 * count how often each landmark was in view and how often it was found, make
 * new landmarks from the triangulated keypoints no landmark claimed, drop the
 * landmarks that do not hold up, and now and then squeeze the dropped ones
 * out.  Every call is asynchronous on `stream`, allocates nothing and never
 * synchronises; SLAM_ERR_ARG (a null pointer is reported by the argument's
 * name) comes before any GPU call.
 *
 * Landmark state.  Beside d_X [x_cap][3] f64 and d_desc [x_cap][32] u8 (16-byte
 * aligned) a landmark has four i32 fields: d_visible (frames it was predicted
 * in view), d_found (frames it was matched in), d_born and d_last (the frames
 * of its first and latest observation).  The count *d_n is a DEVICE i32,
 * clamped to [0, x_cap] wherever it is read.  Landmark i < *d_n is DEAD iff
 * d_X[i][0] is NaN: a dead landmark never projects (xc2 > min_depth is false)
 * and is never valid in slam_pose_refine, so indices stay stable and earlier
 * track rows keep their meaning.  1 <= x_cap <= 1 << 20.
 *
 * 1. Score.  d_uv [batch][x_cap][2] f32, d_good [batch][x_cap] u8 and d_nq
 *    [batch] i32 as ONE run of steps 1-4 of guided matching left them; nq_b
 *    (clamped to [0, x_cap]) is the count that run used, not the current *d_n,
 *    and entries >= nq_b are stale: they are not used.  For every i < x_cap
 *      visible[i] += #{b : i < nq_b, uv[b][i][0] finite}
 *      found[i]   += #{b : i < nq_b, good[b][i] != 0}
 *      last[i]     = max(last[i], frame0 + b) over the b counted in found.
 *    One lane per landmark, a loop over the batch: exact, no atomics.
 *    1 <= batch <= 65535. */
int slam_map_score(const float* d_uv, const uint8_t* d_good, const int32_t* d_nq, int x_cap,
                   int batch, int frame0, int32_t* d_visible, int32_t* d_found, int32_t* d_last,
                   void* stream);

/* 2. Spawn.  d_Xc [batch][p_cap][3] f64 camera-frame points as
 *    slam_triangulate writes them, d_pairs [batch][p_cap][2] i32 whose column 0
 *    is the keypoint index j, d_count [batch] (clamped to [0, p_cap]); d_kp
 *    [batch][kp_cap][5] f32, d_kp_desc [batch][kp_cap][32] u8 (16-byte aligned),
 *    d_nkp [batch] (clamped as in slam_kp_grid); d_owner [batch][kp_cap] i32, the
 *    output of slam_match_unique, read and updated; d_poses [batch][16] f64
 *    camera-to-world (R its 3x3, t its last column); d_spawn [batch] u8, the
 *    frames that may spawn.  Entry (b, k) is a CANDIDATE iff
 *      spawn[b] != 0 and k < count_b,
 *      0 <= j < nkp_b and owner[b][j] == -1,
 *      xc0, xc1, xc2 are finite and z_min < xc2 < z_max (both ends excluded),
 *      no k' < k of the same frame is a candidate with the same j.
 *    Candidates are numbered in order of b, then k; number r gets landmark
 *    i = n0 + r, n0 = *d_n on entry, and is ACCEPTED iff i < x_cap.  For an
 *    accepted candidate, without contraction and left to right,
 *      X[i][c] = R[c][0] xc0 + R[c][1] xc1 + R[c][2] xc2 + t[c]
 *      desc[i] = d_kp_desc[b][j], visible[i] = found[i] = 1,
 *      born[i] = last[i] = frame0 + b, owner[b][j] = i,
 *    and the row [frame0 + b, i, (double)kx_j, (double)ky_j] is appended to
 *    d_rows[b] ([batch][rows_cap][4] f64) at d_rows_count[b] (clamped to [0,
 *    rows_cap]), which grows by the frame's accepted candidates: new indices
 *    exceed all old ones, so rows written by slam_track_rows stay in ascending
 *    landmark order.  rows_cap >= min(x_cap, kp_cap), so rows that hold one
 *    row per owned keypoint cannot overflow (a row past rows_cap is not
 *    written).  Further outputs: *d_n = min(n0 + candidates, x_cap), d_spawned
 *    [batch] i32 the accepted candidates per frame, *d_dropped i32 the
 *    candidates not accepted.
 *    d_ws: slam_map_spawn_workspace_bytes(batch, kp_cap) bytes, 4-byte aligned,
 *    contents irrelevant on entry.  Two launches of one workgroup per frame:
 *    the first races k into a claim word per keypoint (integer atomicMin: the
 *    lowest k wins whatever the arrival order) and counts the frame's
 *    candidates; the second adds up the counts of the frames before its own
 *    and scatters.  1 <= batch <= 1024, 1 <= p_cap <= 1 << 20, 1 <= kp_cap <=
 *    65535; z_min < z_max (NaN refused). */
int slam_map_spawn_workspace_bytes(int batch, int kp_cap, size_t* bytes);
int slam_map_spawn(const double* d_Xc, const int32_t* d_pairs, const int32_t* d_count, int p_cap,
                   const float* d_kp, const uint8_t* d_kp_desc, const int32_t* d_nkp, int kp_cap,
                   int32_t* d_owner, const double* d_poses, const uint8_t* d_spawn, int batch,
                   double z_min, double z_max, int frame0, double* d_X, uint8_t* d_desc,
                   int32_t* d_visible, int32_t* d_found, int32_t* d_born, int32_t* d_last,
                   int32_t* d_n, int x_cap, double* d_rows, int32_t* d_rows_count, int rows_cap,
                   int32_t* d_spawned, int32_t* d_dropped, void* d_ws, size_t ws_size,
                   void* stream);

/* 3. Cull.  A live landmark i < *d_n dies iff (products and the difference in
 *    64 bits)
 *      visible[i] >= min_visible and ratio_den found[i] < ratio_num visible[i], or
 *      now - born[i] >= age and found[i] < min_found.
 *    Dying writes NaN to all three of d_X[i]; dead landmarks are left alone;
 *    *d_nculled i32 = the number that died in this call (zeroed on the stream,
 *    then an integer atomic add).  ratio_num >= 0, ratio_den >= 1. */
int slam_map_cull(double* d_X, const int32_t* d_visible, const int32_t* d_found,
                  const int32_t* d_born, const int32_t* d_n, int x_cap, int now, int min_visible,
                  int ratio_num, int ratio_den, int age, int min_found, int32_t* d_nculled,
                  void* stream);

/* 4. Compact.  STABLE compaction of the live landmarks of [0, *d_n): landmark
 *    i goes to d_remap[i] = the number of live landmarks below it, all six
 *    arrays copied into the *_out arrays (same shapes; an output may not be
 *    its own input).  d_remap [x_cap] i32 is -1 for a dead landmark and for
 *    every i >= *d_n; *d_n_out i32 = the new count (not d_n: the last launch
 *    still reads it).
 *    Blocks of 1024 landmarks count, one workgroup scans the block counts,
 *    the blocks scatter: three launches, no workgroup waits for another (the
 *    block counts live in d_remap between the launches). */
int slam_map_compact(const double* d_X, const uint8_t* d_desc, const int32_t* d_visible,
                     const int32_t* d_found, const int32_t* d_born, const int32_t* d_last,
                     const int32_t* d_n, int x_cap, double* d_X_out, uint8_t* d_desc_out,
                     int32_t* d_visible_out, int32_t* d_found_out, int32_t* d_born_out,
                     int32_t* d_last_out, int32_t* d_remap, int32_t* d_n_out, void* stream);

/*    Track rows after a compaction.  d_rows [batch][rows_cap][4] f64 and
 *    d_count [batch] i32 (clamped to [0, rows_cap]) in the format of
 *    slam_track_rows.  A row whose landmark value v is not in (-1, x_cap), NaN
 *    included, or whose d_remap[(int)v] is -1 is dropped; the others are
 *    written to d_rows_out (not d_rows) in their order with d_remap[(int)v] as
 *    the landmark, and d_count_out [batch] counts them.  1 <= batch, rows_cap
 *    <= 65535. */
int slam_rows_remap(const double* d_rows, const int32_t* d_count, int rows_cap, int batch,
                    const int32_t* d_remap, int x_cap, double* d_rows_out, int32_t* d_count_out,
                    void* stream);

/* 5. Fuse.  Spawn makes a landmark from every triangulated keypoint that no
 *    landmark owns, so a landmark that was in view but failed its match in a
 *    keyframe gets a twin at the same world point; from then on the twins
 *    compete for one keypoint in every frame.  Fuse finds such twins in what
 *    ONE run of steps 1-4 of guided matching left and merges them.
 *    Inputs: d_uv [batch][x_cap][2] f32 and d_z [batch][x_cap] f64 (the xc2
 *    slam_project_landmarks writes), d_idx2 [batch][x_cap][2] i32, d_good0
 *    [batch][x_cap] u8 (step 3's d_good, before the uniqueness pass), d_good
 *    [batch][x_cap] u8 (step 4's d_good_out), d_owner [batch][kp_cap] i32 (after
 *    slam_map_spawn or not), d_nq [batch] i32 (clamped to [0, x_cap]; entries at
 *    or beyond nq_b are stale and not used), and the landmark state with *d_n.
 *    In frame b, (l, w) is a CANDIDATE PAIR iff
 *      l < nq_b, good0[b][l] != 0 and good[b][l] == 0 (l passed the descriptor
 *        tests and lost the keypoint),
 *      0 <= j = idx2[b][l][0] < kp_cap, 0 <= w = owner[b][j] < nq_b, w != l,
 *      l and w are below *d_n and alive,
 *      uv[b][l] and uv[b][w] are finite and du du + dv dv <= px px, du and dv
 *        the f64 differences of the f32 values (left to right, no contraction),
 *      |z[b][l] - z[b][w]| <= rel_depth min(z[b][l], z[b][w]) (false with a NaN),
 *      the Hamming distance of desc[l] and desc[w] is <= max_dist.
 *    RANK: a outranks b iff found[a] > found[b], or they are equal and a < b;
 *    found is read as on entry and a negative value counts as 0.  PARENT[i] is
 *    the best-ranked landmark among i itself and every partner of i in any
 *    candidate pair of any frame, whichever side i was on; a parent strictly
 *    outranks its child, so there is no cycle.  This is the forest of best
 *    partners, NOT connected components: with pairs a-b and b-c where a
 *    outranks c and c outranks b, b goes to a and c stays; a later call
 *    catches c.  root(i) follows parent to its fixed point.
 *    d_to [x_cap] i32 = root(i) for i < *d_n and i for every other index;
 *    landmark i is FUSED iff to[i] != i.  For every fused i with r = to[i]:
 *      visible[r] += visible[i], found[r] += found[i] (the merged found /
 *        visible ratio lies between the two ratios),
 *      born[r] = min(born[r], born[i]), last[r] = max(last[r], last[i]),
 *      all three of d_X[i] become NaN: i is dead exactly as a culled landmark;
 *    desc[i] and i's own counters are left alone, d_X[r] and desc[r] do not
 *    change.  *d_nfused i32 = the number fused in this call.
 *    Three launches.  One lane per landmark writes its own rank key
 *    (INT32_MAX - max(found, 0)) << 32 | i to a u64 word; one lane per (b, l)
 *    does one 64-bit atomicMin of the better key of a pair into the word of
 *    the worse-ranked landmark, so the words do not depend on the order of
 *    arrival; one lane per landmark walks the low halves to its root and
 *    merges with integer atomics on the root's counters.
 *    d_ws: slam_map_fuse_workspace_bytes(x_cap) bytes, 8-byte aligned, contents
 *    irrelevant on entry.  1 <= batch <= 65535, 1 <= kp_cap <= 65535, px > 0,
 *    rel_depth >= 0 (NaN refused), 0 <= max_dist <= 256. */
int slam_map_fuse_workspace_bytes(int x_cap, size_t* bytes);
int slam_map_fuse(const float* d_uv, const double* d_z, const int32_t* d_idx2,
                  const uint8_t* d_good0, const uint8_t* d_good, const int32_t* d_owner,
                  const int32_t* d_nq, int batch, int kp_cap, double* d_X, const uint8_t* d_desc,
                  int32_t* d_visible, int32_t* d_found, int32_t* d_born, int32_t* d_last,
                  const int32_t* d_n, int x_cap, double px, double rel_depth, int max_dist,
                  int32_t* d_to, int32_t* d_nfused, void* d_ws, size_t ws_size, void* stream);

/*    Track rows after a fuse.  d_rows [batch][rows_cap][4] f64 and d_count
 *    [batch] i32 (clamped to [0, rows_cap]) in the format of slam_track_rows;
 *    d_to [x_cap] i32 as slam_map_fuse wrote it.  A row whose landmark value v
 *    is an integer in [0, x_cap) stands for v' = d_to[(int)v]; any other row
 *    (NaN, negative, >= x_cap, not an integer; also one whose d_to entry is
 *    not in [0, x_cap)) is copied as it is and competes with nobody.  Among
 *    the rows of one frame with the same v' exactly one is kept: the row with
 *    v == v' (the survivor's own observation) of the lowest k if there is one,
 *    otherwise the row of the lowest k -- an integer atomicMin of
 *    (v != v' ? 65536 : 0) + k.  The kept rows are written to d_rows_out in
 *    their order with v' as the landmark, and d_count_out [batch] counts them;
 *    an output may not be its own input.  Afterwards the rows of a frame are
 *    no longer in ascending landmark order; slam_points_refine and
 *    slam_pose_refine do not need that order.
 *    d_ws: slam_rows_fuse_workspace_bytes(batch, x_cap) bytes, 4-byte aligned,
 *    contents irrelevant on entry.  1 <= batch, rows_cap <= 65535. */
int slam_rows_fuse_workspace_bytes(int batch, int x_cap, size_t* bytes);
int slam_rows_fuse(const double* d_rows, const int32_t* d_count, int rows_cap, int batch,
                   const int32_t* d_to, int x_cap, double* d_rows_out, int32_t* d_count_out,
                   void* d_ws, size_t ws_size, void* stream);

/* ------------------------------------------------------------------------
 * Structure-only refinement of the landmarks from their tracks: the poses are
 * held and every landmark is refined from all of its observations in a window
 * of frames -- the counterpart of slam_pose_refine, one independent 3x3
 * problem per landmark.  Asynchronous on `stream`; it allocates nothing and
 * never synchronises the host.
 *
 * Inputs.  d_rows [n_frames][rows_cap][4] f64 and d_count [n_frames] i32
 * (clamped to [0, rows_cap]) as slam_track_rows and slam_map_spawn write them;
 * the frame column is not read: the position f in the window names the frame.
 * d_poses [n_frames][16] f64 row-major camera-to-world (R its 3x3, t its last
 * column); d_P [12] f64, a 3x4 projection whose fourth column may be non-zero;
 * d_X [x_cap][3] f64, read and updated in place; *d_n (DEVICE i32, clamped to
 * [0, x_cap]) the landmark count: landmarks at or beyond it are not touched.
 *
 * Observations of landmark i.  For each frame f in ascending order the row
 * k < count_f whose landmark column equals i exactly; if several rows of a
 * frame name i, the one with the lowest k, whatever order they are met in (an
 * integer atomicMin of k, as in slam_map_spawn).  A row whose landmark column
 * is NaN, negative, >= x_cap or not an integer belongs to nobody.  The rows
 * need not be sorted.
 *
 * Model, for the observation (f, x, y) at the point X, in this order and
 * without contraction:
 *   d    = X - t_f
 *   xc_k = R_f[0][k] d0 + R_f[1][k] d1 + R_f[2][k] d2      (slam_project_landmarks)
 *   h_i  = P[i][0] xc0 + P[i][1] xc1 + P[i][2] xc2 + P[i][3]
 *   r    = (h0 (1 / h2) - x, h1 (1 / h2) - y)
 * VALID AT X iff xc2 > min_depth and h2 > 0.  The 2x3 Jacobian is a R_f^T with
 * a = ((P[0,:3] - u P[2,:3]) (1 / h2), (P[1,:3] - v P[2,:3]) (1 / h2)):
 *   J[c][k] = a[c][0] R_f[k][0] + a[c][1] R_f[k][1] + a[c][2] R_f[k][2].
 * loss 0..3 and loss_scale are those of slam_pose_refine: r and J are scaled
 * by sqrt(rho'(z)), z = |r|^2 / delta^2, and the term is delta^2 rho(z) (loss 0:
 * |r|^2).
 *
 * Rounds, per landmark.  A landmark whose d_X[i][0] is NaN is dead: status 4,
 * nothing is written for it.  A_0 = the observations valid at the input point;
 * fewer than min_obs: status 1.  Each of the n_rounds rounds runs `iters`
 * Levenberg-Marquardt iterations with lambda starting at 1e-3: H = sum J^T J,
 * g = sum J^T r and cost = sum term over A IN FRAME ORDER (per observation row
 * 0 of J, then row 1); the step solves (H + lambda max(diag H, 1e-12)) d = -g
 * by a 3x3 Cholesky; the trial X + d is accepted iff the factorisation
 * succeeded, every observation of A is valid at the trial and cost_trial <
 * cost; lambda <- max(lambda / 10, 1e-12) on accept, min(10 lambda, 1e12) on
 * reject.  After each round EVERY observation of the landmark is classified:
 * an inlier iff valid and its unweighted |r|^2 <= gate^2; the inliers are the
 * next round's A; fewer than min_obs of them: status 2, and the rounds end.
 *
 * Guard.  After the last round H is formed over the final inliers at the
 * final point, robust-weighted and undamped, and factored: with L L^T = H and
 * M = L^-1, var = max_i sum_k M[k][i]^2, the largest diagonal entry of H^-1, in
 * m^2 per px^2 of observation variance.  Status 3 iff a pivot is not positive
 * and finite, or var <= max_var is false; max_var = +inf leaves the pivot test
 * alone.  Without the guard a landmark near the axis of motion (no parallax)
 * takes an unconstrained step and is thrown far away: a status-3 landmark
 * keeps its position.
 *
 * Outputs.
 *   d_X                       rewritten only for status 0; for every other
 *                             status the input point stays bit for bit
 *   d_status [x_cap] i32      0 refined; 1 fewer than min_obs observations
 *                             valid at the input point; 2 the inliers fell
 *                             below min_obs after a round; 3 the guard; 4 dead;
 *                             -1 at and beyond *d_n
 *   d_nobs [x_cap] i32        the final inliers (status 0, 3), -1 otherwise
 *   d_cost [x_cap] f64        sum of term over the final inliers at the final
 *                             point (status 0, 3), 0 otherwise
 *   d_info [x_cap][9] f64     that H, row-major and symmetric bit for bit
 *                             (status 0, 3), zeros otherwise: the landmark's
 *                             information matrix
 *   d_var [x_cap] f64         var (status 0, 3; +inf where the factorisation
 *                             failed), 0 otherwise
 *   d_mask [n_frames][rows_cap] u8   1 for a row that is the observation of a
 *                             landmark i < *d_n alive on entry and in its last
 *                             classification (status 1: valid at the input
 *                             point); 0 for every other row below count_f
 *                             (nobody's, the loser among duplicates, a dead
 *                             landmark's); entries >= count_f are not written
 *   d_nkilled [1] i32         with kill != 0 every status-2 landmark dies
 *                             (NaN in all three of d_X[i]) and their number
 *                             goes here (zeroed on the stream, then an integer
 *                             atomic add); with kill == 0 it is not written.
 * d_ws: slam_points_refine_workspace_bytes(n_frames, x_cap) bytes (an i32 per
 * frame and landmark), 4-byte aligned, contents irrelevant on entry.  Two
 * launches: one lane per row races k into the index word [f][i]; one lane per
 * landmark then runs the rounds in its own registers, in frame order, so the
 * result is that of a sequential evaluation.
 * SLAM_ERR_ARG before any GPU call (a null pointer is reported by the
 * argument's name): n_frames outside 1..64; rows_cap outside 1..65535; x_cap
 * < 1; n_rounds outside 1..8; iters outside 1..50; min_obs < 2; loss outside
 * 0..3; loss_scale <= 0 with loss != 0; gate <= 0; min_depth NaN; max_var NaN
 * or <= 0; ws_bytes smaller than the query says. */
int slam_points_refine_workspace_bytes(int n_frames, int x_cap, size_t* bytes);
int slam_points_refine(const double* d_rows, const int32_t* d_count, int rows_cap, int n_frames,
                       const double* d_poses, const double* d_P, double* d_X, const int32_t* d_n,
                       int x_cap, int loss, double loss_scale, double gate, double min_depth,
                       int n_rounds, int iters, int min_obs, double max_var, int kill,
                       int32_t* d_status, int32_t* d_nobs, double* d_cost, double* d_info,
                       double* d_var, uint8_t* d_mask, int32_t* d_nkilled, void* d_ws,
                       size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Relocalization: the pose of a frame in the map WITHOUT a predicted pose --
 * what lost tracking and loop closure need.  The frame's keypoints are matched
 * against the descriptors of all eligible landmarks (no window), every landmark
 * keeps at most one keypoint (slam_match_unique with the roles swapped: queries
 * are keypoints, targets are landmarks, so d_owner [batch][x_cap] names the
 * keypoint a landmark won), the matches become track rows and PnP inputs,
 * slam_pnp_ransac_ws finds a pose among them, and slam_pose_refine refines it
 * and gives its information.  The three steps below are the new ones; each is
 * asynchronous on `stream`, allocates nothing and never synchronises, and
 * SLAM_ERR_ARG (a null pointer is reported by the argument's name) comes before
 * any GPU call.  The map is the landmark state of the life cycle above: d_X,
 * d_desc, d_last and the DEVICE count *d_n; it is only read.
 *
 * 1. Hamming kNN-2 against the live map.  Queries d_q [batch][q_cap][32] u8,
 *    d_nq [batch] i32 (a negative count is 0, otherwise clamped to q_cap); the
 *    map is shared by all items; d_range [batch][2] i32 = (lo_b, hi_b).
 *    Landmark i is ELIGIBLE for item b iff
 *      i < clamp(*d_n, 0, x_cap), d_X[i][0] is not NaN (alive) and
 *      lo_b <= d_last[i] < hi_b.
 *    For query j < nq_b the two smallest (distance, landmark index) pairs over
 *    the eligible landmarks are reported, ties to the lower index:
 *      d_idx2, d_dist2 [batch][q_cap][2] i32: full 32-bit landmark indices,
 *             -1 / -1 where there is none
 *      d_good [batch][q_cap] u8 = 1 iff both exist, d1 <= max_dist and
 *             ratio_den d1 < ratio_num d2.
 *    Two candidates are required, as in slam_hamming_knn2: this is a global
 *    search, not a window.  Rows >= nq_b are not written.  An ineligible
 *    landmark never appears in an output and never affects a ratio; the result
 *    does not depend on the processing order.  d_range and *d_n are read on the
 *    device: a captured graph can be replayed with other ranges and a grown map.
 *    Two launches.  The map is cut into segments of SLAM_MAP_KNN_SEGMENT
 *    landmarks and the grid is (query tile, segment, item), so one frame against
 *    a large map fills the chip; a workgroup writes its queries' top-2 of its
 *    segment to d_ws as dist << 20 | landmark, and the second launch merges the
 *    segments per query and applies the ratio test.
 *    d_ws: slam_hamming_map_workspace_bytes(batch, q_cap, x_cap) bytes (8 per
 *    item, segment and query), 8-byte aligned, contents irrelevant on entry; a
 *    smaller ws_bytes is an argument error that names the needed size.
 *    1 <= x_cap <= 1 << 20, 1 <= q_cap <= 65535, 1 <= batch <= 65535, max_dist
 *    in 0..256, 0 < ratio_num <= ratio_den <= 1 << 20; d_q and d_desc 16-byte
 *    aligned. */
#define SLAM_MAP_KNN_SEGMENT 2048
int slam_hamming_map_segment(void); /* SLAM_MAP_KNN_SEGMENT of the built library */
int slam_hamming_map_workspace_bytes(int batch, int q_cap, int x_cap, size_t* bytes);
int slam_hamming_map_knn2(const uint8_t* d_q, const int32_t* d_nq, int q_cap,
                          const uint8_t* d_desc, const double* d_X, const int32_t* d_last,
                          const int32_t* d_n, int x_cap, const int32_t* d_range, int batch,
                          int max_dist, int ratio_num, int ratio_den, int32_t* d_idx2,
                          int32_t* d_dist2, uint8_t* d_good, void* d_ws, size_t ws_bytes,
                          void* stream);

/* 2. Rows and PnP inputs from the owners.  d_owner [batch][x_cap] i32 as
 *    slam_match_unique wrote it with keypoints as queries and landmarks as
 *    targets; d_kp [batch][kp_cap][5] f32.  For every landmark i < clamp(*d_n,
 *    0, x_cap) with 0 <= j = owner[b][i] < kp_cap, in ascending i, row k gets
 *      d_rows[b][k] = [frame0 + b, i, (double)kx_j, (double)ky_j]
 *      d_Q[b][k]    = d_X[i]                  ([batch][rows_cap][3] f64)
 *      d_q[b][k]    = ((double)kx_j, (double)ky_j)   ([batch][rows_cap][2] f64)
 *    and d_count [batch] i32 counts them: the row format of slam_track_rows (so
 *    slam_pose_refine takes d_rows unchanged) and the inputs of slam_pnp_ransac
 *    with cap = rows_cap.  rows_cap >= min(x_cap, kp_cap) or an argument error.
 *    One workgroup per frame.  1 <= batch <= 65535, 1 <= x_cap <= 1 << 20,
 *    1 <= kp_cap <= 1 << 20. */
int slam_reloc_rows(const int32_t* d_owner, const int32_t* d_n, int x_cap, const float* d_kp,
                    int kp_cap, const double* d_X, int batch, int frame0, int rows_cap,
                    double* d_rows, int32_t* d_count, double* d_Q, double* d_q, void* stream);

/* 3. PnP result -> start pose of the refinement.  d_rvec, d_tvec [batch][3] f64
 *    and d_ninl [batch] i32 as slam_pnp_ransac wrote them with K = d_P[:, :3]
 *    (d_P [12] f64, 3x4, its left 3x3 upper triangular with a non-zero
 *    diagonal: not checked here); d_count [batch] i32 the rows of step 2;
 *    d_prior [batch][16] f64 camera-to-world poses, or NULL for the identity.
 *    With s = K^-1 P[:, 3] by back substitution
 *      s2 = P23 / P22, s1 = (P13 - P12 s2) / P11, s0 = ((P03 - P01 s1) - P02 s2) / P00
 *    a frame with ninl >= min_inliers gets the camera-to-world pose
 *      R' = Rod(rvec)^T, t' = -R' (tvec - s), last row 0 0 0 1,
 *    and d_count_out[b] = d_count[b].  A frame with ninl < min_inliers (-1
 *    included) gets its prior bit for bit and d_count_out[b] = 0:
 *    slam_pose_refine then reports status 1 and returns that pose bit for bit,
 *    so no second status word is needed.  d_poses [batch][16] f64 may not alias
 *    d_prior.  1 <= batch <= 65535, min_inliers >= 0. */
int slam_reloc_pose(const double* d_rvec, const double* d_tvec, const int32_t* d_ninl,
                    const int32_t* d_count, const double* d_P, const double* d_prior, int batch,
                    int min_inliers, double* d_poses, int32_t* d_count_out, void* stream);

/* ------------------------------------------------------------------------
 * Tiled ORB detector + rBRIEF descriptor.
 *
 * Replaces orb_detector_using_tiles (/root/reference/orb.py:4-25), i.e. the
 * per-patch cv2.ORB_create(nfeatures=max_kp, scaleFactor=1.2).detect() +
 * .compute() of orb_extraction_detect (orb.py:28-38), with the OpenCV 4.x ORB
 * semantics restated in oracle/orb.c (bit-exact against it; canonical keypoint
 * order: level, Harris response desc, y, x).  Tiles follow orb.py exactly:
 * tile_h = int(H/height_div), tile_w = int(W/width_div), patches of
 * int(tile + tile/overlap_div) starting at every multiple of the tile size
 * below H - tile_h (resp. W - tile_w), clipped to the image.
 * height_div == width_div == 0 runs ORB on the whole image as one patch
 * (orb_extraction_detect itself); patches must fit the 160 KiB LDS budget.
 *
 *   d_img   [batch][H][stride] u8
 *   d_kp    [batch][kp_cap][5] f32  (x, y, size, angle [deg], response)
 *   d_octave[batch][kp_cap] i32, d_desc [batch][kp_cap][32] u8
 *   d_count [batch] i32: number of keypoints, or -(n)-1 on overflow
 *   d_ws    workspace of slam_orb_workspace_bytes(...) bytes
 * ---------------------------------------------------------------------- */
int slam_orb_workspace_bytes(int batch, int H, int W, int max_kp, int overlap_div,
                             int height_div, int width_div, size_t* bytes);
int slam_orb_tiles(const uint8_t* d_img, int batch, int H, int W, int stride, int max_kp,
                   int overlap_div, int height_div, int width_div, void* d_ws,
                   size_t ws_bytes, float* d_kp, int32_t* d_octave, uint8_t* d_desc,
                   int32_t* d_count, int kp_cap, void* stream);

/* ------------------------------------------------------------------------
 * Bundle adjustment (BAL model) — replaces the reference's BAL block
 * /root/reference/BundleAdjustment.py:287-402 (rotate / project / objective /
 * bundle_adjustment_sparsity / least_squares TRF) with Levenberg-Marquardt on
 * the normal equations: analytic 2x12 Jacobian per observation; per point
 * group (whole points, <= 128 observations) the point blocks are eliminated and
 * the group's share of the reduced camera system (camera Grams U - sum Y W^T,
 * off-diagonal sums Y W^T, Jc^T r, Jc^T u) is written as slot partials that a
 * second launch sums per block in group order (deterministic); blocked LDL^T
 * of the reduced camera system.
 *
 * Camera layout per row: [r0 r1 r2 t0 t1 t2 f k1 k2] (BundleAdjustment.py:324).
 * ---------------------------------------------------------------------- */

/* objective() residuals (BundleAdjustment.py:331-369) in the caller's
 * observation order: d_resid [n_obs][2] (= the reference's ravel order).
 * Indices must be in range (checked by the host wrapper). */
int slam_ba_residual(const double* d_cams, const double* d_pts, const int32_t* d_cam_idx,
                     const int32_t* d_pt_idx, const double* d_qs, int n_obs,
                     double* d_resid, void* stream);

/* Per-observation residual and Jacobian (clamped like objective()):
 * d_jac [n_obs][2][12] columns [w0 w1 w2 t0 t1 t2 f k1 k2 | X0 X1 X2]. */
int slam_ba_jacobian(const double* d_cams, const double* d_pts, const int32_t* d_cam_idx,
                     const int32_t* d_pt_idx, const double* d_qs, int n_obs,
                     double* d_resid, double* d_jac, void* stream);

/* LM state slots (doubles in slam_ba_problem.state). */
#define SLAM_BA_ST_LAMBDA 0
#define SLAM_BA_ST_NU 1
#define SLAM_BA_ST_COST 2      /* 0.5*|r|^2 at the live parameters (with a robust  */
#define SLAM_BA_ST_COST_NEW 3  /* loss: 0.5 d^2 sum rho(z)); at the last trial step */
#define SLAM_BA_ST_PRED 4      /* predicted reduction of the last trial step   */
#define SLAM_BA_ST_RHO 5
#define SLAM_BA_ST_ACCEPTED 6  /* 1 if the last trial step was accepted        */
#define SLAM_BA_ST_CUR 7       /* which of the two parameter buffers is live   */
#define SLAM_BA_ST_ITERS 8
#define SLAM_BA_ST_NACCEPT 9
#define SLAM_BA_ST_PRED_CAM 10
#define SLAM_BA_ST_CHOL_FAIL 11 /* last solve: 0 ok, 1 not SPD, 2 dataflow solve timed out */
/* slots 12..15: the phase timers of the -DSLAM_SOLVE_PROFILE build
 * (scripts/ba_solve_prof.py reads state[12:16]); slots 17..19: unused */
#define SLAM_BA_ST_SOLVE_FAULT 16 /* sticky: camera solves whose dataflow wait timed out
                                     * (fail code 2: a hang or a hand-off ordering bug --
                                     * the solve needs no co-residency, so a correct build
                                     * never sets it; the Python layer raises when non-zero) */
#define SLAM_BA_ST_SLOTS 20

/* Everything the LM iteration touches; all pointers are device pointers.
 * Built by the host planner (slam355/ba_plan.py): observations sorted by
 * (point, camera); index tables are fixed for the life of a problem. */
typedef struct slam_ba_problem {
  int32_t n_cams, n_pts, n_obs;
  int32_t n_grps;        /* point groups (>= 1): <= 128 obs / points each     */
  int32_t n_blocks;      /* upper camera-pair blocks of S: all C(C+1)/2 when
                            9C <= 120, else the diagonal + every pair with a
                            common point (across all ranks), sorted          */
  int32_t n_cslots;      /* (group, camera) slots                             */
  int32_t n_bslots;      /* (group, camera-pair block) slots                  */
  int32_t lin_mode;      /* 0: slot linearisation (k_linearize; groups = point
                            groups); 1: camera-union linearisation
                            (k_lin_mfma; grp_* = chunks, slots per supergroup) */
  int32_t n_sgrps;       /* lin_mode 1: supergroups (>= 1)                    */
  int32_t tl_mode;       /* tiled solve with tl_sched: 0 dataflow (k_tl3_flow,
                            one persistent workgroup per tile column, when the
                            schedule has <= SLAM_TL_FLOW_MAX_T columns), 1 one
                            launch pair per elimination-tree level           */
  double* cams[2];              /* [C][9]  double-buffered, state[CUR] is live */
  double* pts[2];               /* [P][3]                                      */
  double* camrec[2];            /* [C][32] per-camera projection records of cams[] */
  const int32_t* obs_cam;       /* [O] (sorted by point, then camera)          */
  const int32_t* obs_pt;        /* [O]                                         */
  const double* obs_q;          /* [O][2]                                      */
  const int32_t* pt_ptr;        /* [P+1] CSR point -> obs                      */
  const int32_t* grp_ptr;       /* [n_grps+1] point range of each point group  */
  const int32_t* grp_cslot;     /* [n_grps+1] camera-slot range of each group  */
  const int32_t* cslot_cam;     /* [n_cslots] camera of each slot              */
  const int32_t* cslot_obs_ptr; /* [n_cslots+1] range in cslot_obs             */
  const int32_t* cslot_obs;     /* [O] group-local obs indices, slot by slot   */
  const int32_t* grp_bslot;     /* [n_grps+1] block-slot range of each group   */
  const int32_t* bslot_blk;     /* [n_bslots] upper block index (c1 <= c2)     */
  const int32_t* bslot_pair_ptr;/* [n_bslots+1] range in bslot_pairs           */
  const int32_t* bslot_pairs;   /* group-local o1 | o2 << 16, o1 < o2 of one point */
  const int32_t* blocks;        /* [n_blocks][2] (c1 <= c2), every upper block */
  const int32_t* cam_cslot_ptr; /* [C+1] camera -> its rows of cpart            */
  const int32_t* cslot_row;     /* [n_cslots] row of a camera slot in cpart (camera-major, group order) */
  const int32_t* blk_bslot_ptr; /* [n_blocks+1] block -> its rows of bpart (empty: no common point) */
  const int32_t* bslot_row;     /* [n_bslots] row of a block slot in bpart (block-major, group order) */
  double* cpart;                /* [n_cslots][112] U - sum Y W^T (81), Jc^T r, Jc^T u, diag U (9 each), |r|^2 */
  double* bpart;                /* [n_bslots][81] sum Y W^T                    */
  double* sys;                  /* S (dense or packed blocks) b[9C] g[9C] diagU[9C] cost[C] */
  double* chol;                 /* [slam_ba_chol_len] (9C > 120 only)           */
  double* delta_c;              /* [9C]                                        */
  double* red_part;             /* [slam_ba_red_slots(n_grps)]                 */
  double* small;                /* [4] trial |r|^2, sum pred_p (all-reduced)   */
  double* state;                /* [SLAM_BA_ST_SLOTS]                          */
  uint32_t* ticket;             /* [1] zero-initialised completion counter     */
  /* lin_mode 1 only (else may be null): points renumbered by camera span;
   * grp_ptr = chunks (<= 128 obs, <= 16 points); grp_cslot / grp_bslot are
   * indexed by supergroup. */
  const int32_t* sg_ptr;        /* [n_sgrps+1] chunk range of each supergroup    */
  const int32_t* sg_meta;       /* [n_sgrps][24] ch0 ch1 (chunk range), cslot start, m
                                   (cameras), bslot start, count, the first chunk's
                                   point and obs range, its cameras[8] (<= 7, sorted,
                                   -1 padded), pad                              */
  const int32_t* obs_meta;      /* [O] lpt | la << 8 | cobs << 16: chunk-local point,
                                   position of the obs's camera in sg_cams, and the
                                   chunk-local obs list sorted by (la, obs)      */
  const int32_t* chk_optr;      /* [n_grps+1] first observation of each group /
                                   chunk (= pt_ptr[grp_ptr]); required in both modes */
  const int32_t* chk_cptr;      /* [n_grps][8] start of each camera's run in chk_cobs */
  const int32_t* bslot_ab;      /* [n_bslots] camera pair a | b << 8 (a < b) of a block slot */
  /* Level schedule of the tiled solve (required when 9C > 120), built by
   * slam355/ba_plan.py tl_schedule: tiles of whole cameras (64-row tiles, the rows
   * past a tile's cameras padding) in nested-dissection order, with the row
   * maps between S and the tiled system, columns grouped by elimination-tree
   * level, the dataflow solve's column table, epilogue and gather tables and
   * its product task table (12-int header; the layout is tl_schedule's and is
   * checked by the launcher).
   * tl_sched is the device copy, tl_sched_host the same array in host memory
   * (the launcher reads the level counts from it); both or neither. The
   * workspace `chol` is sized from it: slam_ba_chol_len(n_cams, tl_sched_host). */
  const int32_t* tl_sched;
  const int32_t* tl_sched_host;
  /* lin_mode 1, optional (null: the separate k_assemble launch): the assembly
   * folded into k_lin_mfma -- the supergroup that writes the LAST partial row
   * of a block sums that block's rows (deterministic order) into sys.  int32:
   * need[n_blocks] (partial rows per block), cnt[n_blocks] (zero-initialised;
   * re-armed by the assembler), cam_dblk[C] (diagonal block of each camera),
   * row_blk[n_bslots] (block of each bpart row), n_empty, empty[n_empty]
   * (blocks with no partial row here: zeroed every build). */
  int32_t* asm_tab;
  /* Optional (null: all n_blocks): the blocks this problem's assembly runs
   * over -- those with partial rows here (a landmark shard touches few of the
   * global list): asm_act[n_asm_act] ascending block indices, then a 0/1 flag
   * per block (listed or not) and a 0/1 flag per camera (its diagonal block
   * listed).  Those workgroups also write the zeros of the unlisted blocks (S
   * -0.0, and b, g -0.0 / diag U, cost +0.0 for a camera without rows: what
   * the assembly writes for them, up to the sign of a zero on the diagonal of
   * a camera this rank does not observe).  Packed systems (9C > 120) without
   * asm_tab only; n_asm_act >= 1. */
  const int32_t* asm_act;
  int32_t n_asm_act;
  /* Robust loss per observation (was the unused asm_pad; 0 keeps the plain
   * 0.5 |r|^2): 0 linear, 1 huber, 2 soft_l1, 3 cauchy -- scipy's names and
   * rho, applied to the 2-vector reprojection error.  With s = r0^2 + r1^2 of
   * the clamped residual and z = s / loss_scale^2 the observation enters the
   * normal equations as sqrt(w) r and sqrt(w) J (all 12 columns), w = rho'(z)
   * (the Gauss-Newton / IRLS form, no rho'' term), and the LM cost is
   * 0.5 loss_scale^2 sum rho(z) (SLAM_BA_ST_COST / _COST_NEW).  huber: rho =
   * z (z <= 1) or 2 sqrt(z) - 1; soft_l1: 2 (sqrt(1 + z) - 1); cauchy:
   * log(1 + z).  The launchers refuse loss outside 0..3 and, with loss != 0,
   * a loss_scale that is not finite and > 0.  Landmark shards: every rank
   * passes the same loss.  slam_ba_residual / slam_ba_jacobian stay raw. */
  int32_t loss;
  /* Optional (null: every parameter free): held camera parameters, one word
   * per camera [n_cams]; bit i (0..8: w0 w1 w2 t0 t1 t2 f k1 k2) set holds
   * parameter i of that camera constant -- its column leaves the Jacobian
   * (k_linearize / k_lin_mfma drop it from the 2 x 9 camera block of every
   * observation), the LM iteration is otherwise unchanged, and its step is an
   * exact zero (the held row of the reduced system keeps only its damped
   * diagonal, lambda * 1e-6).  Gauge: hold the oldest keyframes whole (0x1FF);
   * a calibrated camera: hold f, k1, k2 (0x1C0).  Landmark shards: every rank
   * passes the same words.  Appended in ABI 1 (slam_abi_version() still
   * returns 1): callers that zero the descriptor keep today's behaviour, and
   * slam_ba_problem_size() tells a binding which layout a library has. */
  double loss_scale;            /* delta of `loss` in pixels (read when loss != 0) */
  const uint32_t* cam_fixed;    /* (documented above loss_scale; stays the last field) */
} slam_ba_problem;
/* sizeof(slam_ba_problem) of this library (400 with cam_fixed, 408 with loss_scale). */
int slam_ba_problem_size(void);

/* Largest tile count (tl_sched[1]) the dataflow tiled solve takes: one
 * persistent workgroup per tile column (they need not all be resident). */
#define SLAM_TL_FLOW_MAX_T 256

/* Problems per batched launch (slam_ba_iterate_batch splits larger batches).
 * The descriptors travel by value in the kernel arguments: 16 x 408 B
 * (ba_common.hpp static_asserts the size; ROCm 7.2 takes this > 4 KB argument
 * segment, exercised by tests/test_ba.py's 16-window launch). */
#ifndef SLAM_BA_MAX_BATCH
#define SLAM_BA_MAX_BATCH 16
#endif

/* ---- host planner of the camera-union linearisation (lin_mode 1) ----------
 * slam355/ba_plan.py plan_mfma in native code (the same tables, element for
 * element; no HIP call, callable without a GPU): observations sorted by
 * (point, camera), points renumbered by camera span, chunks of <= 120
 * observations / 16 points, supergroups of <= chunks_per_wg chunks seeing
 * <= 7 cameras.  Replaces the Python planner that BundleAdjustment-style
 * callers (BundleAdjustment.py:331-402 via slam355.ba.BAProblem) pay per
 * window.  The tables go into one int32 buffer `out`, table k at info->off[k]
 * (256-byte aligned), info->len[k] entries; sizes in info.  info->ok = 0
 * (and SLAM_OK) when a point has > 120 observations or > 7 cameras: the slot
 * linearisation (lin_mode 0) applies.  chunks_per_wg <= 0: the default rule
 * of plan_mfma.  block_list (packed layout, 9C > 120; may be null): the
 * upper blocks to list, as BAProblem's block_list.  Null means "the problem's
 * own blocks"; a non-null pointer with n_block_list == 0 is an explicitly empty
 * list and fails like any list that misses a block (plan_mfma raises alike). */
enum {
  SLAM_PLAN_PERM = 0,      /* [P] device point k = caller's point perm[k]      */
  SLAM_PLAN_ORDER,         /* [O] observation order (qs[order] -> obs_q)       */
  SLAM_PLAN_OBS_CAM, SLAM_PLAN_OBS_PT, SLAM_PLAN_PT_PTR, SLAM_PLAN_GRP_PTR,
  SLAM_PLAN_GRP_CSLOT, SLAM_PLAN_CSLOT_CAM, SLAM_PLAN_GRP_BSLOT, SLAM_PLAN_BSLOT_BLK,
  SLAM_PLAN_BLOCKS, SLAM_PLAN_CAM_CSLOT_PTR, SLAM_PLAN_CSLOT_ROW, SLAM_PLAN_BLK_BSLOT_PTR,
  SLAM_PLAN_BSLOT_ROW, SLAM_PLAN_SG_PTR, SLAM_PLAN_SG_META, SLAM_PLAN_SG_CAMS,
  SLAM_PLAN_OBS_LA, SLAM_PLAN_CHK_COBS, SLAM_PLAN_OBS_META, SLAM_PLAN_CHK_OPTR,
  SLAM_PLAN_CHK_CPTR, SLAM_PLAN_BSLOT_AB,
  SLAM_PLAN_NTAB
};
typedef struct slam_ba_plan_info {
  int32_t ok, n_obs, n_grps, n_sgrps, n_cslots, n_bslots, n_blocks, chunks_per_wg;
  long long off[SLAM_PLAN_NTAB], len[SLAM_PLAN_NTAB];
  long long total;  /* int32 slots written */
} slam_ba_plan_info;
/* int32 slots `out` needs for any plan of this size (0 on bad sizes). */
long long slam_ba_plan_bound(int n_cams, int n_pts, int n_obs, int n_block_list);
int slam_ba_plan_mfma(int n_cams, int n_pts, int n_obs, const int32_t* cam_idx,
                      const int32_t* pt_idx, const int32_t* block_list, int n_block_list,
                      int chunks_per_wg, int32_t* out, long long out_cap,
                      slam_ba_plan_info* info);

/* Host staging of a batch of tracked local-BA windows (the tracked leg's
 * host side in one call; replaces a Python loop over windows, buffers and plan
 * tables -- main.py:120-127 / XXXport_files.py:44-64 build the reference's BA
 * arguments from the local map).  Window w = frames w n .. w n + n - 1 (one
 * camera each, parameters cams[w n + j][9]); observations = the first cnt[b]
 * rows (frame j, map point, u, v) of rows[b][cap][4] for its pairs b, q = (u -
 * u_off, v - v_off); points = maps[w][0 .. M[w])[3].  Each window is planned
 * (slam_ba_plan_mfma) and, when the plan exists and 9n <= 120, its float64
 * data (BAProblem's layout: cams0 pts0 cams1 pts1 init_c init_p obs_q, then
 * zeroed camrec0 camrec1 cpart bpart sys chol delta_c red_part small state,
 * each 32-double aligned) go to h64 and its plan tables (+ 8 zero int32:
 * stand-ins, ticket) to h32; probs[w] gets the device addresses of those
 * buffers at d64 / d32.  meta[w][SLAM_STAGE_META]: staged (0: the caller builds
 * that window itself), C, P, O, n_grps, n_sgrps, n_cslots, n_bslots, n_blocks,
 * int32 offset, plan length, sys length, the SLAM_STAGE_NF64 float64 offsets,
 * the SLAM_PLAN_NTAB table offsets.  need[2] = doubles / int32 used; with
 * null outputs, or when they exceed cap64 / cap32, only sizes and meta are
 * produced (grow the buffers and call again). */
#define SLAM_STAGE_NF64 17
#define SLAM_STAGE_META (12 + SLAM_STAGE_NF64 + SLAM_PLAN_NTAB)
int slam_ba_stage_windows(int n_win, int n, int cap, const double* rows, const int32_t* cnt,
                          const double* maps, int map_cap, const int32_t* M, const double* cams,
                          double u_off, double v_off, double* h64, long long cap64, int32_t* h32,
                          long long cap32, const void* d64, const void* d32,
                          slam_ba_problem* probs, long long* meta, long long* need);
/* The float64 layout of one BA problem (host only, no GPU call): the
 * SLAM_STAGE_NF64 segments in the order listed above, len[k] doubles each
 * (cams 9C, pts 3P, obs_q 2 max(O, 1), camrec 32C, cpart 112 n_cslots, bpart
 * 81 n_bslots, sys slam_ba_sys_len(n_cams, n_blocks), chol chol_len, delta_c
 * 9C, red_part slam_ba_red_slots(n_grps), small 4, state SLAM_BA_ST_SLOTS; a
 * workspace keeps at least one element), off[k] the segment's start relative
 * to the problem's first double (every start a multiple of 32 doubles), *total
 * the aligned length of the whole.  chol_len: slam_ba_chol_len for a tiled
 * solve (9C > 120), 0 otherwise.  slam_ba_stage_windows lays every window out
 * with it; slam355/ba.py allocates BAProblem and BAWindowSet.build from it. */
int slam_ba_f64_layout(int n_cams, int n_pts, int n_obs, int n_grps, int n_cslots, int n_bslots,
                       int n_blocks, long long chol_len, long long len[SLAM_STAGE_NF64],
                       long long off[SLAM_STAGE_NF64], long long* total);
/* The int32 words of one staged problem whose plan has plan_len words: the
 * plan tables, then 8 zero words (from plan_len: the one-element stand-ins of
 * the lin_mode-0 tables; at *ticket = plan_len + 4: the completion ticket;
 * *end = plan_len + 8), rounded up to a multiple of 32.  Returns that length
 * (0 on plan_len < 0); ticket and end may be null. */
long long slam_ba_i32_layout(long long plan_len, long long* ticket, long long* end);

/* Number of doubles red_part needs for a problem with n_grps point groups. */
int slam_ba_red_slots(int n_grps);
/* Doubles of the tiled-Cholesky workspace `chol` (needed only when 9C > 120)
 * for a tile schedule (the host copy tl_sched_host, slam355/ba_plan.py
 * tl_schedule): its tile count tl_sched_host[1] (a schedule of whole-camera
 * tiles may have more tiles than 9C / 64) and its product slots
 * tl_sched_host[11] (the 64x64 terms L_Ik L_Jk^T that column k forms for
 * column J's first two row tiles).  NULL: ceil(9C / 64) tiles, no slots. */
long long slam_ba_chol_len(int n_cams, const int32_t* tl_sched_host);
/* Doubles in the all-reduced system buffer `sys`: dense (9C <= 120) (9C)^2,
 * packed (9C > 120) 81 * n_blocks (the listed upper camera blocks), then
 * b, g, diag U (9C each) and the per-camera cost (C). */
long long slam_ba_sys_len(int n_cams, int n_blocks);

/* Phase 1 (per rank): linearise at the live parameters and build this
 * rank's share of the reduced camera system into prob->sys. */
int slam_ba_build_system(const slam_ba_problem* prob, void* stream);
/* Phase 2 (after sys is summed over ranks): damp, Cholesky-solve for the
 * camera step, back-substitute the point step, evaluate the trial cost
 * partial sums into prob->small. */
int slam_ba_solve_step(const slam_ba_problem* prob, void* stream);
/* Phase 3 (after small is summed over ranks): LM accept/reject, lambda update. */
int slam_ba_decide(const slam_ba_problem* prob, void* stream);
/* Single-rank convenience: n_iter x (phase 1, 2, 3) with no host sync. */
int slam_ba_iterate(const slam_ba_problem* prob, int n_iter, void* stream);
/* Reset the LM state: lambda0, nu = 2, cur = 0, counters = 0. */
int slam_ba_reset(const slam_ba_problem* prob, double lambda0, void* stream);
/* Batched local BA: n_probs independent problems (e.g. the local-BA windows
 * of a tracking batch; the reference solves one BAL problem per call,
 * BundleAdjustment.py:397-402) advance n_iter LM iterations through shared
 * launches, up to SLAM_BA_MAX_BATCH problems per launch (one problem per
 * grid row).  Every problem keeps its own buffers and LM state: its iterates
 * are the ones slam_ba_iterate gives it alone.  Batched problems must use the
 * one-workgroup solver (9C <= 120); a packed problem iterates on its own. */
int slam_ba_iterate_batch(const slam_ba_problem* probs, int n_probs, int n_iter, void* stream);

/* Marginal covariance of the camera parameters: 9x9 blocks of
 * S0^-1, where S0 = U - W V^-1 W^T is the reduced camera system at the live
 * parameters with ZERO damping, built from the same clamped, masked, robust-
 * weighted Jacobian as every LM step -- the camera part of (J^T J)^-1, in the
 * units of unit-variance pixel noise.  d_pairs [n_pairs][2] camera indices
 * (a, b), in range (checked by the host wrapper); d_cov [n_pairs][9][9]
 * row-major, block q = Cov(camera a, camera b) (a == b: a marginal block,
 * exactly symmetric; block (a, b) is block (b, a) transposed bit for bit).
 * Rows and columns of held parameters (cam_fixed) are +0.0.  The caller fixes
 * the gauge (two cameras held whole suffice for the BAL model): d_status[0] = 1
 * and every output NaN when S0 is not numerically positive definite, i.e. a
 * pivot of the unpivoted Cholesky is not finite or L_kk^2 <= rank_tol * S0_kk
 * (rank_tol finite, in [0, 1)); 0 otherwise.  A point whose 3x3 block is
 * singular at lambda = 0 contributes with a zero inverse (as in the LM steps).
 * d_ws: slam_ba_cov_workspace_len(n_cams) doubles (two dense matrices of
 * ceil(9C / 64) 64x64 tile rows), ws_len its length.  Asynchronous on
 * `stream`, no allocation, no host sync; lambda and every other LM state slot
 * are as before afterwards, but prob->sys is overwritten: a
 * slam_ba_build_system made before must be repeated before
 * slam_ba_solve_step (slam_ba_iterate rebuilds anyway).  Single rank: the
 * system of a landmark shard is not summed over ranks here.  The landmark
 * blocks of the same inverse: slam_ba_covariance_points. */
long long slam_ba_cov_workspace_len(int n_cams);
int slam_ba_covariance(const slam_ba_problem* prob, const int32_t* d_pairs, int n_pairs,
                       double rank_tol, double* d_cov, double* d_ws, long long ws_len,
                       int32_t* d_status, void* stream);

/* Camera, landmark and landmark-camera blocks of (J^T J)^-1 from one build
 * and one factorisation.  With Sigma_cc = S0^-1 as above, per
 * observation o of point p and camera c(o) the Jacobian blocks Jc_o (2x9), Jp_o
 * (2x3), W_o = Jc_o^T Jp_o, and V_p = sum_o Jp_o^T Jp_o (no damping):
 *   Sigma_pp[p]    = V_p^-1 + V_p^-1 (sum_{o,o'} W_o^T Sigma_{c(o)c(o')} W_o') V_p^-1   (3x3)
 *   Sigma_pc[p, c] = -V_p^-1 sum_o W_o^T Sigma_{c(o), c}                                (3x9)
 * for any camera c, observing p or not; the sums run over the observations of
 * p, so a repeated (point, camera) pair counts every time.
 *   d_pairs  [n_pairs][2]  -> d_cov    [n_pairs][9][9]   as slam_ba_covariance (n_pairs may be 0)
 *   d_points [n_points]    -> d_cov_pp [n_points][3][3]  point indices in the problem's (device)
 *                             order; d_points NULL with n_points == n_pts: every point in order
 *   d_cross  [n_cross][2]  -> d_cov_pc [n_cross][3][9]   (point, camera)
 * An entry may repeat; each gets its own output row, and a row's bits do not
 * depend on the rest of the request.  Sigma_pp is exactly symmetric; columns
 * of held camera parameters in Sigma_pc are +0.0.  An index out of range gives
 * a NaN row (never a read outside a buffer; the host wrapper checks first).
 * d_status[0]: S0 not positive definite, as slam_ba_covariance (then every
 * output is NaN).  A point is undetermined when a pivot of the unpivoted 3x3
 * Cholesky of V_p is not finite or <= rank_tol * V_kk (no observation, one
 * observation, a degenerate ray bundle): its requested rows are NaN and
 * d_status[1] counts them; d_status[0] is not raised by it.  (S0 itself still
 * takes such a point with the zero inverse of the LM steps when det V = 0 and
 * with a huge inverse otherwise: drop one-observation points from a problem
 * whose camera blocks matter.)
 * Refused before any launch: all three counts 0, a negative count, a non-zero
 * count with a null list or output (except the all-points form), and what
 * slam_ba_covariance refuses for rank_tol and the workspace (the same
 * slam_ba_cov_workspace_len doubles).  Stream, allocation, LM state and
 * prob->sys as slam_ba_covariance. */
int slam_ba_covariance_points(const slam_ba_problem* prob,
                              const int32_t* d_pairs, int n_pairs, double* d_cov,
                              const int32_t* d_points, int n_points, double* d_cov_pp,
                              const int32_t* d_cross, int n_cross, double* d_cov_pc,
                              double rank_tol, double* d_ws, long long ws_len,
                              int32_t* d_status /* [2] */, void* stream);

/* Minimum dynamic LDS (bytes, <= 160 KiB) the one-workgroup camera solve
 * (9C <= 120) requests; 0 (default) = what it needs.  A floor above what
 * co-resident workgroups of other streams leave (e.g. > 80 KiB beside an ORB
 * workgroup) keeps its latency-bound pivot chain on CUs of its own.  Process-wide;
 * takes effect at the next launch (and is baked into graphs captured after). */
int slam_ba_set_solve_lds_floor(int bytes);

/* 1 (default): slam_ba_iterate / slam_ba_iterate_batch let the one-workgroup
 * camera solve (9C <= 120) sum the lineariser's partial rows in its own
 * workgroup, with no k_assemble launch before it, for every launch set in which
 * no problem has asm_tab or asm_act and every problem has at most 1024 partial
 * rows (n_cslots + n_bslots: beyond that one workgroup per window is slower
 * than k_assemble's one per block).  2: the same without the row limit (tests,
 * measurements).  0: the separate k_assemble launch.  sys,
 * state and parameters are the same bits either way; slam_ba_build_system /
 * _solve_step / _decide and the covariance calls always use k_assemble.
 * Process-wide; read when launches are issued (a captured graph keeps what it
 * was captured with). */
int slam_ba_set_fused_assembly(int on);

/* Minimum dynamic LDS (bytes, <= 160 KiB) k_orb_tile requests; 0 (default) =
 * what the patch needs (~79 KiB at C2: two workgroups per CU).  Between 80 and
 * ~80.6 KiB one ORB workgroup per CU leaves room for one local-BA
 * linearisation workgroup beside it.  Process-wide (A/B experiments). */
int slam_orb_set_lds_floor(int bytes);

/* Entries per wave and pyramid level of the corner lists k_orb_tile's FAST pass
 * leaves for its NMS pass; 0 (default) = the wave's full share of the tile's
 * scratch (1251 at C2), a larger value is clipped to that.  A level in which a
 * wave meets more corners than this finds them by scanning the score map
 * instead, with the same result: a small value forces that path on ordinary
 * images (tests, profiling).  Process-wide; takes effect at the next launch. */
int slam_orb_set_corner_cap(int entries_per_wave);

/* *d_min = min(*d_min, d_count[0..n)) on the device (the Tracker's running
 * minimum of slam_orb_tiles' counts: a negative count flags an overflow), with
 * no host round trip. */
int slam_count_min(const int32_t* d_count, int n, int32_t* d_min, void* stream);
int slam_ba_reset_batch(const slam_ba_problem* probs, int n_probs, double lambda0, void* stream);

/* ------------------------------------------------------------------ collectives
 * The sharded local BA (replaces the one serial least_squares
 * call of BundleAdjustment.py:397-402 at C4 / C5 scale): each rank holds the
 * observations of its landmark shard and all cameras; per LM iteration the
 * packed reduced camera system and the 4-double trial buffer are summed over
 * the ranks.  RCCL (over xGMI) is loaded at the first slam_comm_* call
 * (dlopen "librccl.so.1", or SLAM_RCCL_LIB, or an RCCL already exporting the
 * nccl* symbols globally).  One rank per GPU; the communicator is used from
 * one host thread at a time. */
#define SLAM_COMM_ID_BYTES 128
typedef struct slam_comm_opaque* slam_comm_t;
/* Rank 0 creates the id (h_id: SLAM_COMM_ID_BYTES host bytes) and sends it to
 * the other ranks out of band (torch.distributed broadcast, MPI, a file). */
int slam_comm_unique_id(void* h_id);
/* Collective over the nranks processes (ncclCommInitRank); the current HIP
 * device is this rank's GPU. */
int slam_comm_init(int nranks, int rank, const void* h_id, slam_comm_t* comm);
int slam_comm_destroy(slam_comm_t comm);
/* In-place sum over the ranks of d_buf[0..n) (f64), async on stream. */
int slam_comm_allreduce_f64(slam_comm_t comm, double* d_buf, long long n, void* stream);
/* One LM iteration of a landmark-sharded problem (every rank calls it on its
 * shard; prob built with the GLOBAL problem's packed block list): phase 1,
 * all-reduce of prob->sys (slam_ba_sys_len doubles), phase 2, all-reduce of
 * prob->small (4 doubles), phase 3 -- all on `stream`, no host sync.  With
 * nranks = 1 it equals slam_ba_iterate(prob, 1, stream). */
int slam_ba_step_distributed(const slam_ba_problem* prob, slam_comm_t comm, void* stream);

/* ------------------------------------------------------------------ pose chain
 * The live pose-chain optimisation of BundleAdjustment.py:79-183 (loop
 * closure): m relative poses [r0 r1 r2 t0 t1 t2] (cv2.Rodrigues rotation
 * vector, translation), residuals f_i (weighted |.| of the six parameters,
 * :114-127) and, with loop != 0, the two loop-closure residuals of the chained
 * absolute pose (:128-134).  All pointers are device pointers. */

/* resid[v][m (+2)] = objective(params[v]) (or objective_without_loop_closure
 * when loop == 0) for n_vec parameter vectors params[v][6m]; each vector's
 * chain product runs in the reference's order.  Replaces objective /
 * objective_without_loop_closure, BundleAdjustment.py:79-145. */
int slam_pose_chain_objective(const double* params, int n_vec, int n_frames, int loop,
                              double* resid, void* stream);
/* Doubles of the LM workspace for m frames (the live parameters sit at its
 * start: ws[0 .. 6m)). */
long long slam_pose_chain_workspace_len(int n_frames);
/* scipy's TRF (least_squares method='trf', x_scale='jac', 'exact' trust-region
 * subproblem) on ws[0 .. 6m) in place, one workgroup, at most max_iter outer
 * iterations per call (first != 0 starts the run: scale, Delta; else it
 * resumes from state).  Analytic Jacobian; the subproblem's SVD solves are
 * replaced by the O(m) arrow-structured dual system.  m <= 512: every frame's
 * state in the registers of one thread (k_chain_trf_r); larger m: the LDS /
 * workspace form (environment SLAM_CHAIN_TRF=lds selects it for any m).  state[16]: cost0, cost,
 * nfev, njev, status (0 running, 1 gtol, 2 ftol, 3 xtol, 4 ftol+xtol), Delta,
 * alpha, iterations.  Replaces least_squares(objective, ..., method='trf') of
 * bundle_adjustment_with_sparsity, BundleAdjustment.py:179-183. */
int slam_pose_chain_trf(double* ws, int n_frames, int loop, int max_iter, int first, double ftol,
                        double xtol, double gtol, int max_nfev, double* state, void* stream);

/* ------------------------------------------------------------------ SE(3) pose graph
 * A general pose graph: N poses x_i = [r (Rodrigues vector), t],
 * T_i = [R(r_i) | t_i], and E relative-pose edges k = (i, j, z_k, A_k), i != j
 * in either order, repeated pairs allowed.  z_k = [r_z, t_z] measures
 * T_i^-1 T_j; A_k is a 6x6 row-major square-root information matrix (the
 * edge's information is A_k^T A_k).  With E = Z^-1 T_i^-1 T_j the raw residual
 * is e_k = [Log(R_E); t_E], the weighted one r_k = A_k e_k.  Levenberg-Marquardt
 * with additive updates on x and the BA's rules and state slots (SLAM_BA_ST_*:
 * LAMBDA, NU, COST, COST_NEW, PRED, RHO, ACCEPTED, CUR, ITERS, NACCEPT,
 * CHOL_FAIL); the damped normal equations are factored as a row-profile
 * ("skyline") Cholesky over 64x64 f64 tiles of 10 poses each, in keyframe
 * order.  Asynchronous on the caller's stream, no allocation. */
typedef struct slam_pg_problem {
  int32_t n_poses, n_edges;
  int32_t loss;                 /* 0 linear, 1 huber, 2 soft_l1, 3 cauchy, on s = |r_k|^2 (as slam_ba_problem.loss) */
  int32_t sched_len;            /* ints in sched / sched_host */
  double loss_scale;            /* delta of `loss` (read when loss != 0) */
  double* poses[2];             /* [6 N] each; state[SLAM_BA_ST_CUR] names the live one */
  const int32_t* edge_ij;       /* device [2 E]: i, j per edge */
  const int32_t* edge_ij_host;  /* the same on the host (validated before any launch) */
  const double* meas;           /* device [6 E] */
  const double* sqrt_info;      /* device [36 E] */
  const uint32_t* pose_fixed;   /* device [N] or null: bit p holds parameter p (0x3F: the pose whole);
                                 * that column leaves every Jacobian, its step is an exact zero and its
                                 * value is copied, bit for bit, into the trial buffer */
  /* The host-built schedule (slam355.posegraph.pg_schedule), a device and a
   * host copy; the host copy is validated against edge_ij_host before any
   * launch.  Header of 16 ints: magic 0x50473031, N, E, T = ceil(N / 10), the
   * unique unordered pose pairs P, the stored tiles, the total panel rows, the
   * total update pairs, the largest panel and update list of a column.  Then
   * first[T] (the smallest tile column of tile row I), rowoff[T + 1] (tile
   * (I, J) is stored tile rowoff[I] + J - first[I]), pose_ptr[N + 1] and
   * pose_ent[2 E] (pose -> 2 edge + side in edge order), pair_ptr[P + 1],
   * pair_ij[2 P] (lo < hi, sorted) and pair_ent[E] (2 edge + (i > j) in edge
   * order), col_ptr[T + 1], upd_ptr[T + 1], the panel rows {I > k : first[I]
   * <= k} of every column k (ascending) and its update pairs (I, J), I >= J,
   * over those rows. */
  const int32_t* sched;
  const int32_t* sched_host;
  double* ws;                   /* slam_pg_workspace_len doubles */
  long long ws_len;
  double* state;                /* [SLAM_BA_ST_SLOTS] */
} slam_pg_problem;
int slam_pg_problem_size(void);
/* Doubles of ws for N poses, E edges and the schedule's stored tile count. */
long long slam_pg_workspace_len(int n_poses, int n_edges, int n_tiles_stored);
/* state <- (lambda0, nu = 2, CUR = 0, COST at poses[0]). */
int slam_pg_reset(const slam_pg_problem* prob, double lambda0, void* stream);
/* n_iters LM iterations with no host synchronisation.  A factor that is not
 * positive definite sets CHOL_FAIL = 1 and takes a zero step (rejected). */
int slam_pg_iterate(const slam_pg_problem* prob, int n_iters, void* stream);
/* At the live poses: e[E][6] raw and r[E][6] = sqrt(w) A e (either may be
 * null).  ws and sched may be null here and in slam_pg_jacobian; state may be
 * null too, and then poses[0] is read. */
int slam_pg_residual(const slam_pg_problem* prob, double* d_e, double* d_r, void* stream);
/* At the live poses: Ji[E][6][6], Jj[E][6][6] = sqrt(w) A d e / d x_i, x_j with
 * the held columns zero. */
int slam_pg_jacobian(const slam_pg_problem* prob, double* d_Ji, double* d_Jj, void* stream);

/* Covariance of the poses: 6x6 blocks of Sigma = H0^-1, where
 * H0 = J~^T J~ at the live poses with ZERO damping, J~ the robust-weighted,
 * A-weighted Jacobian without the held columns that every LM step uses -- in
 * the unit of the edges' information.  d_pairs [n_pairs][2] pose indices
 * (a, b) with a host copy pairs_host (validated before any launch; the launch
 * geometry is computed from it); d_cov [n_pairs][6][6] row-major, block q =
 * Cov(x_a, x_b).  A block with a == b is exactly symmetric; block (a, b) is
 * block (b, a) transposed bit for bit; an entry may repeat, each gets its own
 * row, and a row's bits do not depend on the rest of the request or on its
 * order.  Rows and columns of held parameters (pose_fixed) are +0.0.  The
 * caller fixes the gauge (one pose held whole suffices): d_status[0] = 1 and
 * every output NaN when H0 is not numerically positive definite, i.e. a pivot
 * of the unpivoted skyline Cholesky is not finite or L_rr^2 <= rank_tol *
 * H0_rr (rank_tol finite, in [0, 1)); 0 otherwise.
 * With c = max(a, b) / 10 and r = min(a, b) / 10 the tile column and row of a
 * request, each distinct c costs one 64-column solve through the skyline
 * factor, forwards from tile row c and backwards down to the smallest r asked
 * of it; all columns share the launches: the factor's + 2 + at most 2 T + 1,
 * T = ceil(N / 10), whatever the request.  d_ws: slam_pg_cov_workspace_len(
 * n_poses, n_cols) doubles for the n_cols distinct tile columns of the request
 * (T tiles of 64x64 each, and the request's tables), ws_len its length.
 * Asynchronous on `stream`, no allocation, no host sync.  prob->ws is
 * overwritten (the edge records, the factor, g, D); the poses and every state
 * slot, lambda included, are kept, and slam_pg_iterate rebuilds all of ws, so
 * an iteration after the call is unaffected.
 * Refused before any launch: everything slam_pg_iterate refuses, a null list,
 * host list, output, workspace or status, n_pairs <= 0, an index out of range,
 * rank_tol not finite or outside [0, 1), and a workspace shorter than
 * slam_pg_cov_workspace_len for the request's columns (SLAM_ERR_WORKSPACE).
 * slam_pg_cov_workspace_len: SLAM_ERR_ARG unless 1 <= n_cols <= T. */
long long slam_pg_cov_workspace_len(int n_poses, int n_cols);
int slam_pg_covariance(const slam_pg_problem* prob, const int32_t* d_pairs, const int32_t* pairs_host,
                       int n_pairs, double rank_tol, double* d_cov /* [n_pairs][6][6] */,
                       double* d_ws, long long ws_len, int32_t* d_status, void* stream);
/* The gate of candidate edges k = (i, j, z_k, A_k), i != j, which need not be
 * edges of the graph (a loop-closure proposal): with e_k, J_i, J_j the raw
 * residual and Jacobians of that edge at the live poses (nothing held, no
 * robust weight, A = I),
 *   P_k = J_i S_ii J_i^T + J_i S_ij J_j^T + (J_i S_ij J_j^T)^T + J_j S_jj J_j^T
 * (exactly symmetric) from the blocks S of Sigma above, R_k = (A_k^T A_k)^-1
 * (d_sqrt_info [n][6][6], null: R = 0), S_k = P_k + R_k and d2_k = e_k^T
 * S_k^-1 e_k, the squared Mahalanobis distance of the proposal from the graph
 * (chi^2 with 6 degrees of freedom for a consistent one).  With zero
 * measurements and no information P_k is the first-order covariance of the
 * relative pose T_i^-1 T_j.  d_d2 [n], d_P [n][6][6], d_e [n][6]: each may be
 * null, not all.  A candidate whose S_k fails rank_tol's rule on its own 6x6
 * Cholesky (both poses held and R = 0), or whose A_k^T A_k is not positive
 * definite, gets d2 = NaN, and d_status[1] counts them; d_status[0] and the
 * NaN outputs after a failed factor as above.  The tile columns of a request
 * are those of both poses of every candidate.  Workspace, stream, what is
 * overwritten and kept, and the refusals as slam_pg_covariance; also refused:
 * a candidate with i == j, a null d_meas. */
int slam_pg_gate(const slam_pg_problem* prob, const int32_t* d_cand_ij, const int32_t* cand_ij_host,
                 const double* d_meas, const double* d_sqrt_info /* nullable: R = 0 */, int n_cand,
                 double rank_tol, double* d_d2, double* d_P, double* d_e /* each nullable, not all */,
                 double* d_ws, long long ws_len, int32_t* d_status /* [2] */, void* stream);

/* ------------------------------------------------------------------ BoW
 * Bag-of-words place recognition (bag_of_words.py).  Descriptors are ORB rows
 * (32 bytes, used as float64 features as scikit-learn converts them); K <= 128
 * clusters, centres [K][32] f64.  All pointers are device pointers. */

/* Labels (nearest centre, argmin |c|^2 - 2 x.c, first index on ties) and label
 * histograms hist[n_img][K] of desc[n_img][cap][32] with count[n_img] rows
 * each (count null: n_each rows each); labels may be null.  Replaces
 * BoW.hist (bag_of_words.py:24-27: kmeans.predict + np.histogram). */
int slam_bow_histograms(const uint8_t* desc, const int32_t* count, int n_each, int n_img, int cap,
                        const double* centers, int n_clusters, int32_t* labels, int32_t* hist,
                        void* stream);
/* For each query histogram q: argmin / min over database rows [0, n_db[q]) of
 * sum 2 (x - y)^2 / max(1, x + y) (numpy's summation order; first index on
 * ties; n_db <= 0 -> (-1, -1)).  Replaces the chi2 loop + np.argmin/np.min of
 * BoW.predict_previous / predict (bag_of_words.py:30-56). */
int slam_bow_query(const int32_t* qhist, int n_query, const int32_t* db, const int32_t* n_db,
                   int n_clusters, int32_t* idx, double* val, void* stream);
/* n_iter Lloyd iterations (E-step, then centres = means; an empty cluster keeps
 * its centre) on X[n_points][32] in place on centers (centers_tmp: [K][32]
 * scratch), then labels of the final centres; shift[K] (optional) = squared
 * centre shift of the last iteration.  Replaces KMeans.fit's Lloyd loop
 * (bag_of_words.py:20). */
int slam_bow_lloyd(const uint8_t* X, int n_points, double* centers, double* centers_tmp,
                   int n_clusters, int n_iter, int32_t* labels, double* shift, void* stream);

/* ---------------------------------------------------------------------------
 * Alternative stereo-VO front end: FAST on tiles,
 * pyramidal Lucas-Kanade, semi-global block matching, disparity lookup and
 * float32 triangulation (csrc/vofront.hip; semantics in oracle/vofront.c).
 * ------------------------------------------------------------------------- */

/* Workspace bytes of slam_fast_tiles. */
int slam_fast_tiles_workspace_bytes(int batch, int H, int W, int tile_h, int tile_w, int per_tile,
                                    size_t* bytes);
/* FAST-9/16 (threshold, strict 3x3 NMS) on every tile_h x tile_w tile of
 * img[batch][H][stride]; per tile the detection-order corners, or the first
 * per_tile of a stable sort by response when there are more; tiles row-major.
 * kp[batch][kp_cap][3] f32 (x, y, response), count[batch] (-n-1 if > kp_cap).
 * Replaces VisualOdometry.get_tiled_keypoints (visual_odometry.py:84-96:
 * cv2.FastFeatureDetector_create().detect per tile, sorted(...)[:10]). */
int slam_fast_tiles(const uint8_t* d_img, int batch, int H, int W, int stride, int tile_h,
                    int tile_w, int threshold, int per_tile, void* d_ws, size_t ws_bytes,
                    float* d_kp, int32_t* d_count, int kp_cap, void* stream);

/* Levels actually used and bytes of one image's LK pyramid (the derivative
 * buffer of one image holds img_bytes int16x2 elements). */
int slam_lk_pyramid_layout(int H, int W, int win, int max_level, int* nlev, size_t* img_bytes);
/* Pyramids (pyrDown levels with a reflect-101 border of win+1) of n_img images
 * into d_pyr[n_img][img_bytes]; if d_deriv is not null, also their Scharr
 * derivatives (zero border) into d_deriv[n_img][img_bytes][2].  The pyramid
 * half of cv2.calcOpticalFlowPyrLK (visual_odometry.py:100, keypoint.py:19). */
int slam_lk_build_pyramids(const uint8_t* d_img, int n_img, int H, int W, int stride, int win,
                           int max_level, uint8_t* d_pyr, int16_t* d_deriv, void* stream);
/* Pyramidal LK for pair b = (prev image b * pair_stride_imgs of d_prev_pyr /
 * d_prev_deriv, next image b * pair_stride_imgs of d_next_pyr): points
 * pts[batch][cap][pts_stride] (x, y first), npts[batch] ->
 * out[batch][cap][2], status[batch][cap], err[batch][cap] (mean |diff|).
 * Replaces cv2.calcOpticalFlowPyrLK(img1, img2, pts, None, winSize=(win,win),
 * maxLevel, criteria=(EPS|COUNT, max_count, eps)) (visual_odometry.py:26-29,100). */
int slam_lk_track(const uint8_t* d_prev_pyr, const int16_t* d_prev_deriv, const uint8_t* d_next_pyr,
                  long long pair_stride_imgs, int batch, int H, int W, int win, int max_level,
                  int max_count, double eps, float min_eig, const float* d_pts, int pts_stride,
                  const int32_t* d_npts, int cap, float* d_out, uint8_t* d_status, float* d_err,
                  void* stream);
/* The filters after the LK call, order-preserving: status, err < max_error,
 * np.around(p2) inside (y < H, x < W; also > 0 when lower_bounds) ->
 * tp1/tp2[batch][cap][2] f32, idx (source index, may be null), count[batch].
 * Replaces visual_odometry.py:102-112 (lower_bounds 0) and keypoint.py:20-32
 * (lower_bounds 1). */
int slam_lk_filter(const float* d_p1, int p1_stride, const float* d_p2, const uint8_t* d_status,
                   const float* d_err, const int32_t* d_npts, int cap, int batch, int H, int W,
                   float max_error, int lower_bounds, float* d_tp1, float* d_tp2, int32_t* d_idx,
                   int32_t* d_count, void* stream);

/* Workspace bytes of slam_sgbm. */
int slam_sgbm_workspace_bytes(int batch, int H, int W, int min_disp, int num_disp, int block,
                              size_t* bytes);
/* Semi-global block matching (MODE_SGBM, 5 directions, BT cost on the
 * Sobel-prefiltered and raw images, uniqueness 0, left-right check 1, 3x3
 * median) of left/right[batch][H][stride] -> disp[batch][H][W] int16 (x16) and,
 * if not null, disp_f32 = disp / 16.  num_disp 32 or 64, min_disp in [0, 64].
 * Replaces cv2.StereoSGBM_create(...).compute(l, r) (visual_odometry.py:22-24,191). */
int slam_sgbm(const uint8_t* d_left, const uint8_t* d_right, int batch, int H, int W, int stride,
              int min_disp, int num_disp, int block, int P1, int P2, void* d_ws, size_t ws_bytes,
              int16_t* d_disp, float* d_disp_f32, void* stream);
/* calculate_right_qs + calc_3d for pair b (visual_odometry.py:114-134): disp1 =
 * d_disp + b * disp1_stride, disp2 = disp1 + disp2_offset (f32 maps [H][W]);
 * (int) truncation and NumPy's negative-index wrap; min_disp < d < max_disp;
 * q*_r = q*_l - (d, 0); Q1/Q2 = f32 homogeneous DLT points divided in f32.
 * Optional f64 copies (q1l64/q2l64, Q1_64/Q2_64, in pairs) feed
 * slam_vo_estimate_pose. */
int slam_vo_right_qs_3d(const float* d_tp1, const float* d_tp2, const int32_t* d_cnt, int cap,
                        int batch, const float* d_disp, long long disp1_stride,
                        long long disp2_offset, int H, int W, float min_disp, float max_disp,
                        const double* d_Pl, const double* d_Pr, float* d_q1l, float* d_q1r,
                        float* d_q2l, float* d_q2r, float* d_Q1, float* d_Q2, double* d_q1l64,
                        double* d_q2l64, double* d_Q1_64, double* d_Q2_64, int32_t* d_count,
                        void* stream);
/* cv2.triangulatePoints on float32 points (the homogeneous result in float32)
 * followed by Q[:3] / Q[3] in float32 (calc_3d, visual_odometry.py:129-134):
 * ptl/ptr[batch][cap][2] f32, count[batch] -> X[batch][cap][3] f32. */
int slam_triangulate_f32(const float* d_ptl, const float* d_ptr, const int32_t* d_count, int cap,
                         int batch, const double* d_Pl, const double* d_Pr, float* d_X,
                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SLAM355_H */
