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
on a narrower search at the refined pose.
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
    device; `add` appends (sizes known on the host).  `observe` projects the
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
        self.n = 0
        self.rows_cap = max(min(self.cap, self.kp_cap), 1)   # track rows of one frame
        self._bufs = {}      # batch size -> the device buffers of observe
        self._rbufs = {}     # batch size -> the device buffers of localize
        self._tracks = []    # (rows, count) of every observe call
        self.uv = self.z = self.idx2 = self.dist2 = self.good = self.owner = None
        self.first = self.cost = None

    def add(self, X, desc):
        """Append landmarks: X [k,3] f64, desc [k,32] u8 (host arrays or tensors)."""
        X = to_dev(X, torch.float64).reshape(-1, 3)
        desc = to_dev(desc, torch.uint8).reshape(-1, 32)
        k = int(X.shape[0])
        if int(desc.shape[0]) != k:
            raise ValueError("LandmarkMap.add: X and desc differ in length")
        if self.n + k > self.cap:
            raise ValueError(f"LandmarkMap.add: capacity {self.cap} < {self.n} + {k}")
        self.X[self.n:self.n + k] = X
        self.desc[self.n:self.n + k] = desc
        self.n += k
        return self

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
        f64, count [B] i32) on the device.  `uv`, `z`, `idx2`, `dist2`, `good`
        (after the uniqueness pass) and `owner` stay as attributes; they are
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
            b["nq"].fill_(self.n)
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

    def reset_tracks(self):
        """Forget the rows kept for `tracks()` (the landmarks stay)."""
        self._tracks = []

    def tracks(self, compact=False):
        """Synchronises: the rows of every observe call so far, concatenated
        ([n,4] f64: frame, landmark, x, y) -- problem_from_map's optimization
        matrix.  With compact=True the landmarks that were never observed are
        left out: returns (rows with the landmark column renumbered, ids) where
        ids [k] are the map indices, so X[ids] are the problem's points."""
        out = [np.zeros((0, 4))]
        for rows, count in self._tracks:
            r, c = rows.cpu().numpy(), count.cpu().numpy()
            out += [r[i, :c[i]] for i in range(len(c))]
        om = np.concatenate(out, 0)
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
