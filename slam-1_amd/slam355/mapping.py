"""Device-resident landmark map: appendKeyPoints (/root/reference/keypoint.py:101-122)
on the GPU.

`MapStore` keeps the map Qs [cap, 3] f64 and its size M in HBM.  `append`
associates one frame's new absolute points with the map (exact nearest
neighbour + the reference's |rel|-scaled gate) and appends the unmatched ones,
all on the stream, so a sequence of frames runs without host synchronisation;
the host only tracks an upper bound of M to size grids and grow the buffer.

`LandmarkMap` keeps a descriptor per landmark as well and re-observes landmarks
by projection: project the map with the predicted pose, search each landmark's
descriptor among the keypoints in a window round its predicted pixel
(slam_project_landmarks ... slam_track_rows; no counterpart in the reference).
`LandmarkMap.localize` turns the matches back into poses: robust motion-only
refinement from the predicted pose (slam_pose_refine), twice, the second time
on a narrower search at the refined pose.  `score`, `spawn`, `cull` and
`compact` let the map follow the camera (slam_map_score ... slam_map_compact):
the landmark count lives on the device, so `step` -- localize, score, spawn
from the keyframes, cull -- runs a batch of frames without a synchronisation.
`fuse` merges the duplicates the spawn makes (slam_map_fuse, slam_rows_fuse):
two landmarks that compete for one keypoint become one with the merged track.
`LandmarkMap.relocalize` needs no predicted pose: a global Hamming search
against the live landmarks (slam_hamming_map_knn2), PnP-RANSAC and the same
refinement -- for lost tracking and for the measurement of a loop edge.
`LandmarkMap.refine_points` is the other half of the alternation `localize`
begins: with the poses held, every landmark is refined from all of its kept
observations in a window of frames (slam_points_refine), on the stream.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, geometry, matcher
from .device import ptr, require_gpu, stream_ptr, to_dev


class MapStore:
    def __init__(self, capacity=1 << 16, max_queries=4096, Qs=None):
        self.dev = require_gpu()
        self.cap = int(capacity)
        self.max_q = int(max_queries)
        self.map = torch.zeros((self.cap, 3), dtype=torch.float64, device=self.dev)
        self.M = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        self.m_bound = 0
        self._ws = None
        self._ws_for = (-1, -1)
        if Qs is not None and len(Qs):
            Qs = np.ascontiguousarray(Qs, np.float64).reshape(-1, 3)
            self._grow(len(Qs))
            self.map[: len(Qs)] = torch.from_numpy(Qs).to(self.dev)
            self.M.fill_(len(Qs))
            self.m_bound = len(Qs)

    def _grow(self, need):
        if need <= self.cap:
            return
        cap = max(need, 2 * self.cap)
        m = torch.zeros((cap, 3), dtype=torch.float64, device=self.dev)
        m[: self.cap] = self.map
        self.map, self.cap = m, cap

    def _workspace(self, n):
        key = (n, self.m_bound)
        if self._ws is None or self._ws_for[0] < n or self._ws_for[1] < self.m_bound:
            nb = ctypes.c_size_t(0)
            _lib.call("slam_map_workspace_bytes", max(n, self.max_q), max(self.m_bound, self.cap),
                      ctypes.byref(nb))
            self._ws = torch.empty(int(nb.value), dtype=torch.uint8, device=self.dev)
            self._ws_for = (max(n, self.max_q), max(self.m_bound, self.cap))
        return self._ws, key

    def append(self, abs_pts, rel_pts, pts2d, frame_index, threshold=0.01, count=None,
               rows=None, stream=None):
        """One frame: abs_pts, rel_pts [N,3] f64, pts2d [N,2] f64 (device) ->
        rows [N,4] f64 = [frame, landmark index, u, v]; the map grows in place.
        `count` (device int32 [1], optional) = number of valid points (<= N)."""
        N = int(abs_pts.shape[0])
        self._grow(self.m_bound + N)
        ws, _ = self._workspace(N)
        out = rows if rows is not None else torch.empty((max(N, 1), 4), dtype=torch.float64,
                                                        device=self.dev)
        _lib.call("slam_map_associate", ptr(self.map), ptr(self.M), self.cap, self.m_bound,
                  ptr(abs_pts), ptr(rel_pts), ptr(pts2d), ptr(count), N, float(threshold),
                  int(frame_index), ptr(out), ptr(ws), ws.numel(), stream_ptr(stream))
        self.m_bound += N
        return out[:N]

    def size(self) -> int:
        """Synchronises: the current number of landmarks."""
        m = int(self.M.item())
        self.m_bound = m
        return m

    def points(self) -> torch.Tensor:
        return self.map[: self.size()]


class LandmarkMap:
    """Landmarks with descriptors, matched to new frames by projection.

    X [capacity,3] f64 world points and desc [capacity,32] u8 live on the
    device, with visible / found / born / last [capacity] i32 and the count
    `n_dev` (int32 [1]) beside them; `add` appends (sizes known on the host),
    `spawn` appends on the device.  `n` is the count on the host: exact while
    only `add` and `compact` change the map, an upper bound after a `spawn`
    until `size()` reads `n_dev`.  A landmark that `cull` dropped keeps its
    index with a NaN position until `compact`.  `observe` projects the
    map into a batch of frames with their predicted poses, searches every
    landmark's descriptor among the keypoints within `radius` pixels of its
    predicted position, gives each keypoint to at most one landmark and returns
    the matches as [frame, landmark, x, y] rows -- the rows MapStore.append
    writes, so `tracks()` feeds XXXport_files.problem_from_map directly.  All
    of it runs on the stream without a host synchronisation."""

    def __init__(self, capacity, kp_cap, W, H, P, cell=32):
        self.dev = require_gpu()
        self.cap, self.kp_cap = int(capacity), int(kp_cap)
        self.W, self.H, self.cell = int(W), int(H), int(cell)
        self.P = to_dev(np.ascontiguousarray(P, np.float64).reshape(3, 4))
        self.X = torch.zeros((self.cap, 3), dtype=torch.float64, device=self.dev)
        self.desc = torch.zeros((self.cap, 32), dtype=torch.uint8, device=self.dev)
        self.visible, self.found, self.born, self.last = (
            torch.zeros((self.cap,), dtype=torch.int32, device=self.dev) for _ in range(4))
        self.n = 0
        self.n_dev = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        self._exact = True   # n == n_dev (False between a spawn and the next size())
        self._alt = None     # the other half of compact's ping-pong buffers
        self._life = {}      # batch size -> the device buffers of spawn
        self._nq = None      # the nq of the last observe
        self.remap = self.nculled = self.spawned = self.dropped = None
        self.rows_cap = max(min(self.cap, self.kp_cap), 1)   # track rows of one frame
        self._bufs = {}      # batch size -> the device buffers of observe
        self._rbufs = {}     # batch size -> the device buffers of localize
        self._reloc = {}     # batch size -> the device buffers of relocalize
        self._P_host = np.ascontiguousarray(P, np.float64).reshape(3, 4).copy()
        self.pnp = self.start = self.matched = None   # relocalize: PnP's outputs, start poses, row counts
        self._tracks = []    # (rows, count) of every observe call
        self._kept_poses = {}  # index into _tracks -> the poses step(refine=...) returned for it
        self._pbufs = {}     # window shape -> the device buffers of refine_points
        self.pt_status = self.pt_nobs = self.pt_cost = self.pt_info = self.pt_var = None
        self.pt_mask = self.pt_nkilled = None
        self.uv = self.z = self.idx2 = self.dist2 = self.good = self.owner = None
        self.good0 = None    # the window search's good, before the uniqueness pass (fuse reads it)
        self._fbufs = {}     # batch size -> the device buffers of fuse
        self.nfused = self.to = None
        self.first = self.cost = None

    def add(self, X, desc, frame=0):
        """Append landmarks: X [k,3] f64, desc [k,32] u8 (host arrays or tensors),
        first seen in `frame` (visible = found = 1, born = last = frame, what
        `spawn` gives a new landmark).  After a `spawn` it synchronises (`size`)."""
        X = to_dev(X, torch.float64).reshape(-1, 3)
        desc = to_dev(desc, torch.uint8).reshape(-1, 32)
        k = int(X.shape[0])
        if int(desc.shape[0]) != k:
            raise ValueError("LandmarkMap.add: X and desc differ in length")
        n = self.size()
        if n + k > self.cap:
            raise ValueError(f"LandmarkMap.add: capacity {self.cap} < {n} + {k}")
        self.X[n:n + k] = X
        self.desc[n:n + k] = desc
        self.visible[n:n + k] = 1
        self.found[n:n + k] = 1
        self.born[n:n + k] = int(frame)
        self.last[n:n + k] = int(frame)
        self.n = n + k
        self.n_dev.fill_(self.n)
        return self

    def size(self) -> int:
        """The number of landmark slots in use, dead ones included.  Synchronises
        after a `spawn`; otherwise the host already knows it."""
        if not self._exact:
            self.n = int(self.n_dev.item())
            self._exact = True
        return self.n

    def _buffers(self, B):
        b = self._bufs.get(B)
        if b is None:
            i32 = dict(dtype=torch.int32, device=self.dev)
            kp0 = torch.zeros((B, self.kp_cap, 5), dtype=torch.float32, device=self.dev)
            b = dict(
                nq=torch.zeros((B,), **i32),
                uv=torch.full((B, self.cap, 2), float("nan"), dtype=torch.float32, device=self.dev),
                z=torch.zeros((B, self.cap), dtype=torch.float64, device=self.dev),
                qr=torch.zeros((B, self.cap), dtype=torch.float32, device=self.dev),
                grid=matcher.KeypointGrid(kp0, torch.zeros((B,), **i32), self.W, self.H, self.cell),
                idx2=torch.full((B, self.cap, 2), -1, **i32),
                dist2=torch.full((B, self.cap, 2), -1, **i32),
                good0=torch.zeros((B, self.cap), dtype=torch.uint8, device=self.dev),
                good=torch.zeros((B, self.cap), dtype=torch.uint8, device=self.dev),
                owner=torch.full((B, max(self.kp_cap, 1)), -1, **i32),
            )
            self._bufs[B] = b
        return b

    def observe(self, frame0, poses, kp, desc, n_kp, radius=15.0, max_dist=64, ratio=(7, 10),
                margin=0.0, min_depth=0.1, stream=None):
        """poses [B,4,4] f64 camera-to-world (predicted), kp [B,kp_cap,5] f32,
        desc [B,kp_cap,32] u8, n_kp [B] i32 -> (rows [B,min(capacity,kp_cap),4]
        f64, count [B] i32) on the device.  `uv`, `z`, `idx2`, `dist2`, `good0`
        (before) and `good` (after the uniqueness pass) and `owner` stay as attributes; they are
        overwritten by the next call of the same batch size."""
        return self._observe(frame0, poses, kp, desc, n_kp, radius, max_dist, ratio, margin,
                             min_depth, stream)

    def _observe(self, frame0, poses, kp, desc, n_kp, radius, max_dist, ratio, margin, min_depth,
                 stream, out=None):
        """observe; with out = (rows, count) it writes there and keeps nothing for tracks()."""
        B = int(poses.shape[0])
        if tuple(kp.shape) != (B, self.kp_cap, 5) or tuple(desc.shape) != (B, self.kp_cap, 32):
            raise ValueError("LandmarkMap.observe: kp / desc do not match (B, kp_cap)")
        b = self._buffers(B)
        with torch.cuda.stream(stream):  # the fills below follow the current stream
            b["nq"].copy_(self.n_dev.expand(B))
            b["qr"].fill_(float(radius))
            uv, z = geometry.project_landmarks(self.X, b["nq"], poses, self.P, self.W, self.H,
                                               margin=margin, min_depth=min_depth,
                                               out=(b["uv"], b["z"]))
            grid = b["grid"].build(kp, n_kp)
            idx2, dist2, good0 = matcher.window_knn2_batch(
                self.desc, uv, b["qr"], b["nq"], desc, kp, n_kp, grid, max_dist=max_dist,
                ratio=ratio, out=(b["idx2"], b["dist2"], b["good0"]))
            owner, good = matcher.unique_matches(idx2, dist2, good0, b["nq"], self.kp_cap,
                                                 out=(b["owner"], b["good"]))
            if out is None:
                # fresh outputs per call: the caller keeps them while later frames run
                rows = torch.zeros((B, self.rows_cap, 4), dtype=torch.float64, device=self.dev)
                count = torch.zeros((B,), dtype=torch.int32, device=self.dev)
            else:
                rows, count = out
            matcher.track_rows(idx2, good, b["nq"], kp, frame0, out=(rows, count))
        self.uv, self.z, self.idx2, self.dist2, self.good, self.owner = uv, z, idx2, dist2, good, owner
        self.good0 = good0
        self._nq = b["nq"]
        if out is None:
            self._tracks.append((rows, count))
        return rows, count

    def _refine_buffers(self, B):
        b = self._rbufs.get(B)
        if b is None:
            f64 = dict(dtype=torch.float64, device=self.dev)
            i32 = dict(dtype=torch.int32, device=self.dev)

            def outs():  # the six outputs of geometry.refine_pose
                return (torch.zeros((B, 4, 4), **f64),
                        torch.zeros((B, self.rows_cap), dtype=torch.uint8, device=self.dev),
                        torch.zeros((B,), **i32), torch.zeros((B,), **i32),
                        torch.zeros((B, 6, 6), **f64), torch.zeros((B,), **f64))
            b = dict(rows=torch.zeros((B, self.rows_cap, 4), **f64), count=torch.zeros((B,), **i32),
                     first=outs(), second=outs())
            self._rbufs[B] = b
        return b

    def localize(self, frame0, poses, kp, desc, n_kp, radius=(15.0, 5.0), max_dist=64,
                 ratio=(7, 10), margin=0.0, min_depth=0.1, stream=None, **refine_options):
        """Track the map from predicted poses: observe with radius[0] and refine the
        poses on those matches (geometry.refine_pose, its options in
        `refine_options`), then observe again with radius[1] at the refined poses
        and refine once more.  A frame whose first refinement fails (status != 0)
        keeps its predicted pose for the second pass.  Only the second pass's rows
        are kept for `tracks()`.

        -> (poses [B,4,4] f64, rows, count, mask [B,rows_cap] u8, ninl [B] i32,
        status [B] i32, info [B,6,6] f64), the last four of the second
        refinement.  rows and count are fresh tensors as observe returns them;
        the others are per-batch-size buffers, overwritten by the next call of
        the same batch size, as are `first` (the six outputs of the first
        refinement) and `cost`.  One stream, no host synchronisation: after a
        first call has allocated the buffers it can be captured in a graph."""
        B = int(poses.shape[0])
        b = self._refine_buffers(B)
        obs = (max_dist, ratio, margin, min_depth, stream)
        with torch.cuda.stream(stream):
            rows, count = self._observe(frame0, poses, kp, desc, n_kp, radius[0], *obs,
                                        out=(b["rows"], b["count"]))
            first = geometry.refine_pose(rows, count, self.X, self.n, poses, self.P,
                                         min_depth=min_depth, out=b["first"], **refine_options)
            rows, count = self._observe(frame0, first[0], kp, desc, n_kp, radius[1], *obs)
            po, mask, ninl, status, info, cost = geometry.refine_pose(
                rows, count, self.X, self.n, first[0], self.P, min_depth=min_depth,
                out=b["second"], **refine_options)
        self.first, self.cost = first, cost
        return po, rows, count, mask, ninl, status, info

    def _reloc_buffers(self, B, n_hyp):
        b = self._reloc.get(B)
        if b is None:
            f64 = dict(dtype=torch.float64, device=self.dev)
            i32 = dict(dtype=torch.int32, device=self.dev)
            u8 = dict(dtype=torch.uint8, device=self.dev)
            b = dict(
                range=torch.zeros((B, 2), **i32),
                ws=matcher.map_knn2_workspace(B, self.kp_cap, self.cap, self.dev),
                idx2=torch.full((B, self.kp_cap, 2), -1, **i32),
                dist2=torch.full((B, self.kp_cap, 2), -1, **i32),
                good0=torch.zeros((B, self.kp_cap), **u8), good=torch.zeros((B, self.kp_cap), **u8),
                owner=torch.full((B, self.cap), -1, **i32),
                Q=torch.zeros((B, self.rows_cap, 3), **f64), q=torch.zeros((B, self.rows_cap, 2), **f64),
                pnp=(torch.zeros((B, 3), **f64), torch.zeros((B, 3), **f64), torch.zeros((B,), **i32),
                     torch.zeros((B, self.rows_cap), **u8)),
                K=self.P[:, :3].contiguous(), n_hyp=0,
                start=torch.zeros((B, 4, 4), **f64), matched=torch.zeros((B,), **i32),
                refine=(torch.zeros((B, 4, 4), **f64), torch.zeros((B, self.rows_cap), **u8),
                        torch.zeros((B,), **i32), torch.zeros((B,), **i32),
                        torch.zeros((B, 6, 6), **f64), torch.zeros((B,), **f64)),
            )
            self._reloc[B] = b
        if b["n_hyp"] < n_hyp:   # the PnP workspace and scratch, held per batch size
            b["pnp_ws"] = geometry.pnp_workspace(B, n_hyp, self.dev)
            b["pnp_scratch"] = geometry.pnp_scratch(B, n_hyp, self.dev)
            b["n_hyp"] = n_hyp
        return b

    def relocalize(self, frame0, kp, desc, n_kp, last_range=None, prior=None, max_dist=64,
                   ratio=(7, 10), seed=0, item0=0, min_inliers=10, pnp=None, keep_tracks=False,
                   stream=None, **refine_options):
        """The poses of a batch of frames in the map without predicted poses: for
        lost tracking and loop closure.  Every keypoint is matched against all
        eligible landmarks (slam_hamming_map_knn2: alive, and `last` inside
        `last_range`), every landmark keeps at most one keypoint
        (slam_match_unique, keypoints as queries), the matches become track rows
        and PnP inputs (slam_reloc_rows), PnP-RANSAC finds a pose among them
        (slam_pnp_ransac_ws with K = P[:, :3], seed, item0 and `pnp` over
        geometry.PNP_DEFAULTS), slam_reloc_pose turns it into the start pose and
        geometry.refine_pose (its options in `refine_options`) refines it.

        kp [B,kp_cap,5] f32, desc [B,kp_cap,32] u8, n_kp [B] i32.  last_range:
        None (every landmark; INT32_MAX itself excluded), one (lo, hi) for all
        frames, or an int32 [B,2] array or tensor; a device tensor is used as it
        is, so a captured graph reads its current contents.  prior [B,4,4] f64
        camera-to-world (None: the identity): what a frame whose PnP finds fewer
        than min_inliers inliers comes back with, bit for bit, at status 1.

        -> (poses [B,4,4] f64, rows, count, mask [B,rows_cap] u8, ninl [B] i32,
        status [B] i32, info [B,6,6] f64) as `localize` returns them; count is 0
        for a frame whose PnP failed.  rows and count are fresh tensors, the
        others per-batch-size buffers overwritten by the next call of the same
        batch size, as are `matched` (the rows written per frame, PnP's count),
        `pnp` (rvec, tvec, ninl, mask of the PnP stage) and `start` (the poses
        handed to the refinement).
        keep_tracks=True appends the rows to those `tracks()` returns.  The map
        is not changed, nor what `observe` left for `score` and `spawn`.  One
        stream, no host synchronisation: after a first call has allocated the
        buffers it can be captured in a graph (host arrays for last_range or
        prior are uploaded at every call; pass device tensors then).  The map's
        capacity is bounded by slam_match_unique's t_cap (65535)."""
        B = int(kp.shape[0])
        if tuple(kp.shape) != (B, self.kp_cap, 5) or tuple(desc.shape) != (B, self.kp_cap, 32):
            raise ValueError("LandmarkMap.relocalize: kp / desc do not match (B, kp_cap)")
        if self.cap > 65535:
            raise ValueError(f"LandmarkMap.relocalize: capacity {self.cap} > 65535 (slam_match_unique)")
        K = self._P_host[:, :3]
        if not np.all(np.isfinite(self._P_host)) or np.any(np.tril(K, -1) != 0.0) or \
                np.any(np.diag(K) == 0.0):
            raise ValueError("LandmarkMap.relocalize: P[:, :3] must be upper triangular with a "
                             "non-zero diagonal (PnP runs with K = P[:, :3])")
        prm = dict(geometry.PNP_DEFAULTS, **(pnp or {}))
        b = self._reloc_buffers(B, int(prm["n_hyp"]))
        if prior is not None:
            prior = to_dev(prior, torch.float64)
            if tuple(prior.shape) != (B, 4, 4):
                raise ValueError("LandmarkMap.relocalize: prior must be [B,4,4]")
        with torch.cuda.stream(stream):
            if isinstance(last_range, torch.Tensor) and last_range.is_cuda:
                rng = last_range
                if rng.dtype != torch.int32 or tuple(rng.shape) != (B, 2):
                    raise ValueError("LandmarkMap.relocalize: a device last_range must be int32 [B,2]")
            else:
                rng = b["range"]
                if last_range is None:
                    last_range = (-(1 << 31), (1 << 31) - 1)
                lr = np.asarray(last_range)
                if lr.shape == (2,):
                    rng[:, 0].fill_(int(lr[0]))
                    rng[:, 1].fill_(int(lr[1]))
                elif lr.shape == (B, 2):
                    rng.copy_(torch.from_numpy(np.ascontiguousarray(lr, np.int32)))
                else:
                    raise ValueError("LandmarkMap.relocalize: last_range is None, (lo, hi) or [B,2]")
            idx2, dist2, good0 = matcher.map_knn2_batch(
                desc, n_kp, self.desc, self.X, self.last, self.n_dev, rng, max_dist=max_dist,
                ratio=ratio, ws=b["ws"], out=(b["idx2"], b["dist2"], b["good0"]))
            owner, _ = matcher.unique_matches(idx2, dist2, good0, n_kp, self.cap,
                                              out=(b["owner"], b["good"]))
            # fresh outputs per call: the caller keeps them while later frames run
            rows = torch.zeros((B, self.rows_cap, 4), dtype=torch.float64, device=self.dev)
            count = torch.zeros((B,), dtype=torch.int32, device=self.dev)
            _lib.call("slam_reloc_rows", ptr(owner), ptr(self.n_dev), self.cap, ptr(kp), self.kp_cap,
                      ptr(self.X), B, int(frame0), self.rows_cap, ptr(rows), ptr(b["matched"]),
                      ptr(b["Q"]), ptr(b["q"]), stream_ptr(None))
            rvec, tvec, pn, _ = geometry.pnp_ransac(
                b["Q"], b["q"], b["matched"], b["K"], seed=seed, item0=item0, out=b["pnp"], ws=b["pnp_ws"],
                scratch=b["pnp_scratch"], **prm)
            _lib.call("slam_reloc_pose", ptr(rvec), ptr(tvec), ptr(pn), ptr(b["matched"]), ptr(self.P),
                      ptr(prior), B, int(min_inliers), ptr(b["start"]), ptr(count), stream_ptr(None))
            # n_x = capacity: the rows name landmarks below the device count only
            po, mask, ninl, status, info, _ = geometry.refine_pose(
                rows, count, self.X, self.cap, b["start"], self.P, min_inliers=min_inliers,
                out=b["refine"], **refine_options)
        self.pnp, self.start, self.matched = b["pnp"], b["start"], b["matched"]
        if keep_tracks:
            self._tracks.append((rows, count))
        return po, rows, count, mask, ninl, status, info

    def reset_tracks(self):
        """Forget the rows kept for `tracks()` (the landmarks stay)."""
        self._tracks = []
        self._kept_poses = {}

    # ------------------------------------------------------------ life cycle
    def _fields(self):
        return self.X, self.desc, self.visible, self.found, self.born, self.last

    def score(self, frame0, stream=None):
        """Count the last `observe` (in `localize`: its second pass) into visible /
        found / last: slam_map_score on the uv, good and nq that call left."""
        if self.uv is None:
            raise ValueError("LandmarkMap.score: no observe call to score")
        _lib.call("slam_map_score", ptr(self.uv), ptr(self.good), ptr(self._nq), self.cap,
                  int(self.uv.shape[0]), int(frame0), ptr(self.visible), ptr(self.found),
                  ptr(self.last), stream_ptr(stream))

    def _life_buffers(self, B):
        b = self._life.get(B)
        if b is None:
            nb = ctypes.c_size_t(0)
            _lib.call("slam_map_spawn_workspace_bytes", B, self.kp_cap, ctypes.byref(nb))
            b = dict(ws=torch.empty(int(nb.value), dtype=torch.uint8, device=self.dev),
                     spawned=torch.zeros((B,), dtype=torch.int32, device=self.dev),
                     dropped=torch.zeros((1,), dtype=torch.int32, device=self.dev))
            self._life[B] = b
        return b

    def spawn(self, frame0, poses, Xc, pairs, count, kp, desc, n_kp, keyframe,
              z_range=(0.1, 70.0), rows=None, rows_count=None, stream=None):
        """New landmarks from the triangulated keypoints no landmark owns
        (slam_map_spawn): Xc [B,p_cap,3] f64 camera-frame points, pairs
        [B,p_cap,2] i32 (column 0 the keypoint) and count [B] i32 as
        Tracker.track leaves X, f_pairs and f_cnt; kp, desc, n_kp the frames'
        keypoints; poses [B,4,4] camera-to-world; keyframe [B] u8, the frames that
        may spawn; z_range the accepted depth (70 m: the reference's
        close_def_in_m).  It reads and updates the `owner` of the last observe and
        appends the new landmarks' rows to `rows` / `rows_count`, by default the
        tensors that observe returned, so the spawning observation is in
        `tracks()`.  -> (spawned [B] i32, dropped [1] i32: candidates that found no
        room), per-batch-size buffers.  No synchronisation: `n` becomes an upper
        bound until `size()`."""
        B = int(poses.shape[0])
        if self.owner is None or int(self.owner.shape[0]) != B:
            raise ValueError("LandmarkMap.spawn: no observe call of this batch size")
        if rows is None:
            if not self._tracks:
                raise ValueError("LandmarkMap.spawn: no kept observe rows; pass rows and rows_count")
            rows, rows_count = self._tracks[-1]
        p_cap = int(Xc.shape[1])
        if tuple(Xc.shape) != (B, p_cap, 3) or tuple(pairs.shape) != (B, p_cap, 2) or \
                tuple(kp.shape) != (B, self.kp_cap, 5) or tuple(desc.shape) != (B, self.kp_cap, 32):
            raise ValueError("LandmarkMap.spawn: Xc / pairs / kp / desc do not match (B, p_cap, kp_cap)")
        if int(rows.shape[0]) != B:
            raise ValueError("LandmarkMap.spawn: rows of another batch size")
        b = self._life_buffers(B)
        keyframe = to_dev(keyframe, torch.uint8)
        _lib.call("slam_map_spawn", ptr(Xc), ptr(pairs), ptr(count), p_cap, ptr(kp), ptr(desc),
                  ptr(n_kp), self.kp_cap, ptr(self.owner), ptr(poses), ptr(keyframe), B,
                  float(z_range[0]), float(z_range[1]), int(frame0), ptr(self.X), ptr(self.desc),
                  ptr(self.visible), ptr(self.found), ptr(self.born), ptr(self.last),
                  ptr(self.n_dev), self.cap, ptr(rows), ptr(rows_count), int(rows.shape[1]),
                  ptr(b["spawned"]), ptr(b["dropped"]), ptr(b["ws"]), b["ws"].numel(),
                  stream_ptr(stream))
        self.n, self._exact = self.cap, False   # a bound that also holds for a graph's replays
        self.spawned, self.dropped = b["spawned"], b["dropped"]
        return self.spawned, self.dropped

    def cull(self, now, min_visible=4, ratio=(1, 4), age=4, min_found=2, stream=None):
        """Drop the landmarks that do not hold up (slam_map_cull): found in fewer
        than ratio of at least min_visible predicted views, or found fewer than
        min_found times `age` frames after birth.  Their position becomes NaN;
        their index stays.  -> nculled [1] i32 (device)."""
        if self.nculled is None:
            self.nculled = torch.zeros((1,), dtype=torch.int32, device=self.dev)
        _lib.call("slam_map_cull", ptr(self.X), ptr(self.visible), ptr(self.found), ptr(self.born),
                  ptr(self.n_dev), self.cap, int(now), int(min_visible), int(ratio[0]),
                  int(ratio[1]), int(age), int(min_found), ptr(self.nculled), stream_ptr(stream))
        return self.nculled

    def compact(self, stream=None):
        """Squeeze the dead landmarks out (slam_map_compact; the order of the
        others is kept), renumber the kept track tensors (slam_rows_remap) and read
        the new count: synchronises.  -> remap [capacity] i32, the new index of
        every old one or -1.  What the last observe left (uv, owner, ...) still
        speaks of the old indices: score and spawn before compacting."""
        if self._alt is None:
            self._alt = tuple(torch.zeros_like(t) for t in self._fields())
            self.remap = torch.full((self.cap,), -1, dtype=torch.int32, device=self.dev)
        with torch.cuda.stream(stream):
            n_out = torch.zeros_like(self.n_dev)
            _lib.call("slam_map_compact", *(ptr(t) for t in self._fields()), ptr(self.n_dev),
                      self.cap, *(ptr(t) for t in self._alt), ptr(self.remap), ptr(n_out),
                      stream_ptr(stream))
            self.n_dev.copy_(n_out)   # in place: a captured graph keeps reading this tensor
            old = self._fields()
            self.X, self.desc, self.visible, self.found, self.born, self.last = self._alt
            self._alt = old
            kept = []
            for rows, count in self._tracks:
                out = (torch.zeros_like(rows), torch.zeros_like(count))
                _lib.call("slam_rows_remap", ptr(rows), ptr(count), int(rows.shape[1]),
                          int(rows.shape[0]), ptr(self.remap), self.cap, ptr(out[0]), ptr(out[1]),
                          stream_ptr(stream))
                kept.append(out)
            self._tracks = kept
            self.n, self._exact = int(self.n_dev.item()), True
        return self.remap

    def _fuse_buffers(self, B):
        b = self._fbufs.get(B)
        if b is None:
            nb = ctypes.c_size_t(0)
            _lib.call("slam_map_fuse_workspace_bytes", self.cap, ctypes.byref(nb))
            b = dict(ws=torch.empty(int(nb.value), dtype=torch.uint8, device=self.dev),
                     to=torch.zeros((self.cap,), dtype=torch.int32, device=self.dev),
                     nfused=torch.zeros((1,), dtype=torch.int32, device=self.dev), rows_ws={})
            self._fbufs[B] = b
        return b

    def _rows_fuse_ws(self, b, B):
        """The claim words of slam_rows_fuse for kept rows of B frames."""
        ws = b["rows_ws"].get(B)
        if ws is None:
            nr = ctypes.c_size_t(0)
            _lib.call("slam_rows_fuse_workspace_bytes", B, self.cap, ctypes.byref(nr))
            ws = torch.empty(int(nr.value), dtype=torch.uint8, device=self.dev)
            b["rows_ws"][B] = ws
        return ws

    def fuse(self, px=3.0, rel_depth=0.1, max_dist=64, rewrite_tracks=True, stream=None):
        """Merge duplicate landmarks (slam_map_fuse): a landmark that passed the
        descriptor tests of the last `observe` (in `localize`: its second pass)
        but lost its keypoint to another landmark that projects within `px`
        pixels of it, at a depth within `rel_depth` of its own and with a
        descriptor within `max_dist` bits, is its duplicate.  Of the two the one
        found more often survives (ties: the lower index); it takes the other's
        visible / found counts and the wider born / last span, keeps its own
        position and descriptor, and the other dies as a culled landmark does.
        With rewrite_tracks every kept (rows, count) goes through slam_rows_fuse
        into fresh tensors, so the survivor carries the merged track (one row
        per frame; the positions in the list stay).  -> (nfused [1] i32, to
        [capacity] i32: the survivor of every landmark, itself if not fused),
        buffers held per capacity and batch size, also kept as `nfused` / `to`.

        What the last observe left (`uv`, `owner`, ...) still speaks of the
        fused indices as if they were alive: score and spawn before fusing.  A
        later `compact` squeezes the fused landmarks out with no further work.
        No host synchronisation; `n` is untouched."""
        if self.uv is None or self.good0 is None:
            raise ValueError("LandmarkMap.fuse: no observe call to fuse from")
        B = int(self.uv.shape[0])
        b = self._fuse_buffers(B)
        _lib.call("slam_map_fuse", ptr(self.uv), ptr(self.z), ptr(self.idx2), ptr(self.good0),
                  ptr(self.good), ptr(self.owner), ptr(self._nq), B, self.kp_cap, ptr(self.X),
                  ptr(self.desc), ptr(self.visible), ptr(self.found), ptr(self.born), ptr(self.last),
                  ptr(self.n_dev), self.cap, float(px), float(rel_depth), int(max_dist), ptr(b["to"]),
                  ptr(b["nfused"]), ptr(b["ws"]), b["ws"].numel(), stream_ptr(stream))
        if rewrite_tracks:
            with torch.cuda.stream(stream):
                kept = []
                for rows, count in self._tracks:
                    ws = self._rows_fuse_ws(b, int(rows.shape[0]))
                    out = (torch.zeros_like(rows), torch.zeros_like(count))
                    _lib.call("slam_rows_fuse", ptr(rows), ptr(count), int(rows.shape[1]),
                              int(rows.shape[0]), ptr(b["to"]), self.cap, ptr(out[0]), ptr(out[1]),
                              ptr(ws), ws.numel(), stream_ptr(stream))
                    kept.append(out)
                self._tracks = kept
        self.nfused, self.to = b["nfused"], b["to"]
        return self.nfused, self.to

    def step(self, frame0, poses, kp, desc, n_kp, Xc, pairs, count, keyframe, z_range=(0.1, 70.0),
             cull=None, refine=None, fuse=None, stream=None, **localize_options):
        """One batch of frames through the map: `localize` from the predicted
        poses, `score` its second pass, `spawn` at the refined poses from the
        frames with keyframe != 0 and status 0, `cull` at now = frame0 + B - 1
        (`cull`: a dict of its options).  -> what `localize` returns.  One stream,
        no host synchronisation: after a first call has allocated the buffers it
        can be captured in a graph.

        fuse: None, or a dict of `fuse`'s options ({}: its defaults).  With a dict
        the duplicates are merged after the spawn and before the cull, so the
        merged counts decide the survivor's fate; the kept track tensors are
        replaced by fresh ones (rewrite_tracks), which a captured graph would
        not follow.

        refine: None, or a dict of `window` (the number of step calls to look
        back, this one included; default 1) and any option of `refine_points`.
        With a dict the call keeps a copy of the poses it returns beside its track
        rows and, after the cull, refines the landmarks over the rows and poses of
        the last `window` calls that were made with `refine` (`refine_points`).
        The window's tensors change from call to call and the copy is a fresh
        tensor, so `step` with `refine` is not meant for graph capture;
        `refine_points` called with fixed tensors is."""
        B = int(poses.shape[0])
        with torch.cuda.stream(stream):
            res = self.localize(frame0, poses, kp, desc, n_kp, stream=stream, **localize_options)
            self.score(frame0, stream=stream)
            flags = (to_dev(keyframe, torch.uint8).ne(0) & res[5].eq(0)).to(torch.uint8)
            self.spawn(frame0, res[0], Xc, pairs, count, kp, desc, n_kp, flags, z_range=z_range,
                       stream=stream)
            if fuse is not None:
                self.fuse(stream=stream, **fuse)
            self.cull(frame0 + B - 1, stream=stream, **(cull or {}))
            if refine is not None:
                opts = dict(refine)
                window = int(opts.pop("window", 1))
                if window < 1:
                    raise ValueError("LandmarkMap.step: refine['window'] must be >= 1")
                last = len(self._tracks) - 1
                self._kept_poses[last] = res[0].clone()
                held = []
                while len(held) < window and last - len(held) in self._kept_poses:
                    held.insert(0, self._kept_poses[last - len(held)])
                for k in [k for k in self._kept_poses if k <= last - window]:
                    del self._kept_poses[k]     # no later window reaches them
                self.refine_points(held, stream=stream, **opts)
        return res

    def _points_buffers(self, shape):
        b = self._pbufs.get(shape)
        if b is None:
            F = sum(shape)
            f64 = dict(dtype=torch.float64, device=self.dev)
            i32 = dict(dtype=torch.int32, device=self.dev)
            b = dict(rows=torch.zeros((F, self.rows_cap, 4), **f64), count=torch.zeros((F,), **i32),
                     poses=torch.zeros((F, 4, 4), **f64),
                     out=(torch.zeros((self.cap,), **i32), torch.zeros((self.cap,), **i32),
                          torch.zeros((self.cap,), **f64), torch.zeros((self.cap, 3, 3), **f64),
                          torch.zeros((self.cap,), **f64),
                          torch.zeros((F, self.rows_cap), dtype=torch.uint8, device=self.dev),
                          torch.zeros((1,), **i32)),
                     ws=geometry.points_workspace(F, self.cap, self.dev))
            self._pbufs[shape] = b
        return b

    def refine_points(self, poses, loss="huber", loss_scale=2.4477, gate=2.4477, min_depth=0.1,
                      n_rounds=3, iters=8, min_obs=3, max_var=0.25, kill=False, stream=None):
        """Refine the landmarks from their kept observations with the poses held
        (geometry.refine_points; structure-only BA, the counterpart of `localize`).

        poses: a list of [B_j,4,4] f64 camera-to-world tensors, each going with one
        of the LAST len(poses) entries of the kept track tensors (the (rows, count)
        pairs behind `tracks()`, one per observe / localize / step call), oldest
        first; at most 64 frames in all.  The rows, counts and poses are
        concatenated on the stream into buffers held per window shape, X is updated
        in place for the landmarks that come out with status 0, and the outputs
        stay as attributes: `pt_status`, `pt_nobs`, `pt_cost`, `pt_info`, `pt_var`
        [capacity...], `pt_mask` [frames,rows_cap] u8 in the order of the window,
        `pt_nkilled` [1] i32 (written with kill=True only).  -> pt_status.
        The kept rows are renumbered by `compact`, so it works after one.  No
        host synchronisation: after a first call of the same window shape has
        allocated the buffers, a call with the same tensors can be captured in a
        graph."""
        poses = list(poses)
        if not self._tracks:
            raise ValueError("LandmarkMap.refine_points: no kept tracks")
        if not poses or len(poses) > len(self._tracks):
            raise ValueError(f"LandmarkMap.refine_points: {len(poses)} pose tensors for "
                             f"{len(self._tracks)} kept track entries")
        kept = self._tracks[-len(poses):]
        shape = tuple(int(r.shape[0]) for r, _ in kept)
        for p, B in zip(poses, shape):
            if tuple(p.shape) != (B, 4, 4):
                raise ValueError(f"LandmarkMap.refine_points: poses {tuple(p.shape)} beside kept "
                                 f"rows of {B} frames")
        if sum(shape) > 64:
            raise ValueError(f"LandmarkMap.refine_points: {sum(shape)} frames > 64")
        if any(int(r.shape[1]) != self.rows_cap for r, _ in kept):
            raise ValueError("LandmarkMap.refine_points: kept rows of another rows_cap")
        b = self._points_buffers(shape)
        with torch.cuda.stream(stream):
            o = 0
            for (rows, count), p, B in zip(kept, poses, shape):
                b["rows"][o:o + B].copy_(rows)
                b["count"][o:o + B].copy_(count)
                b["poses"][o:o + B].copy_(to_dev(p, torch.float64))
                o += B
            out = geometry.refine_points(
                b["rows"], b["count"], b["poses"], self.P, self.X, self.n_dev, loss=loss,
                loss_scale=loss_scale, gate=gate, min_depth=min_depth, n_rounds=n_rounds, iters=iters,
                min_obs=min_obs, max_var=max_var, kill=kill, out=b["out"], workspace=b["ws"])
        (self.pt_status, self.pt_nobs, self.pt_cost, self.pt_info, self.pt_var, self.pt_mask,
         self.pt_nkilled) = out
        return self.pt_status

    def tracks(self, compact=False, drop_dead=True):
        """Synchronises: the rows of every observe call so far, concatenated
        ([n,4] f64: frame, landmark, x, y) -- problem_from_map's optimization
        matrix.  With drop_dead the rows of landmarks that `cull` dropped are left
        out.  With compact=True the landmarks that were never observed are
        left out: returns (rows with the landmark column renumbered, ids) where
        ids [k] are the map indices, so X[ids] are the problem's points."""
        out = [np.zeros((0, 4))]
        for rows, count in self._tracks:
            r, c = rows.cpu().numpy(), count.cpu().numpy()
            out += [r[i, :c[i]] for i in range(len(c))]
        om = np.concatenate(out, 0)
        if drop_dead and len(om):
            dead = np.isnan(self.X[:, 0].cpu().numpy())
            l = om[:, 1].astype(np.int64)
            inside = (l >= 0) & (l < self.cap)
            om = om[~(inside & dead[np.where(inside, l, 0)])]
        if not compact:
            return om
        ids, inv = np.unique(om[:, 1].astype(np.int64), return_inverse=True)
        om[:, 1] = inv.reshape(-1)
        return om, ids


def appendKeyPoints(Qs, absPoint, threshold, points_2d, frame_index, rel_point):
    """(keypoint.py:101-122) -> (Qs with the new landmarks appended, rows [N,4])."""
    Qs = np.asarray(Qs, np.float64).reshape(-1, 3)
    absPoint = np.ascontiguousarray(absPoint, np.float64).reshape(-1, 3)
    rel = np.ascontiguousarray(rel_point, np.float64).reshape(-1, 3)
    p2 = np.ascontiguousarray(points_2d, np.float64).reshape(-1, 2)
    n = len(absPoint)
    store = MapStore(capacity=max(len(Qs) + n, 1), max_queries=max(n, 1), Qs=Qs)
    if n == 0:
        return Qs.copy(), np.empty((0, 4))
    rows = store.append(to_dev(absPoint), to_dev(rel), to_dev(p2[:n]), frame_index, threshold)
    return store.points().cpu().numpy(), rows.cpu().numpy()
