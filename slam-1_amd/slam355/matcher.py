"""Exact Hamming kNN-2 matcher on the GPU (replaces FLANN-LSH knnMatch(k=2)).

Reference call sites: /root/reference/keypoint.py:40-51,
/root/reference/Point3D.py:35-49, /root/reference/tracking.py:14-30.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .device import ptr, require_gpu, stream_ptr, to_dev


def knn2_batch(q: torch.Tensor, nq: torch.Tensor, t: torch.Tensor, nt: torch.Tensor,
               *, out=None, stream=None):
    """Batched kNN-2 + ratio test on device tensors.

    q: [B, q_cap, 32] u8, nq: [B] i32, t: [B, t_cap, 32] u8, nt: [B] i32.
    Returns (idx2 [B,q_cap,2] i32, dist2 [B,q_cap,2] i32, good [B,q_cap] u8).
    Rows >= nq[b] are left untouched (initialised to -1 / 0 when allocated here).
    """
    B, q_cap, _ = q.shape
    t_cap = t.shape[1]
    if out is None:
        idx2 = torch.full((B, q_cap, 2), -1, dtype=torch.int32, device=q.device)
        dist2 = torch.full((B, q_cap, 2), -1, dtype=torch.int32, device=q.device)
        good = torch.zeros((B, q_cap), dtype=torch.uint8, device=q.device)
    else:
        idx2, dist2, good = out
    _lib.call("slam_hamming_knn2", ptr(q), ptr(nq), q_cap, ptr(t), ptr(nt), t_cap, B,
              ptr(idx2), ptr(dist2), ptr(good), stream_ptr(stream))
    return idx2, dist2, good


def compact_matches(idx2, good, nq, *, gate_xyz=None, gate=0.0, out=None, stream=None):
    """Order-preserving list of good (queryIdx, trainIdx) pairs per batch item."""
    B, q_cap = good.shape
    if out is None:
        pairs = torch.empty((B, max(q_cap, 1), 2), dtype=torch.int32, device=good.device)
        count = torch.empty((B,), dtype=torch.int32, device=good.device)
    else:
        pairs, count = out
    _lib.call("slam_compact_matches", ptr(idx2), ptr(good), ptr(nq), q_cap, B,
              ptr(gate_xyz), float(gate), ptr(pairs), ptr(count), stream_ptr(stream))
    return pairs, count


class KeypointGrid:
    """Cell index of a batch of keypoint sets (slam_kp_grid): keypoints binned
    into `cell` x `cell` pixel squares, CSR in row-major cell order.

    kp [B, kp_cap, 5] f32 (x, y first: the layout orb_batch returns), n_kp [B]
    i32.  `cell_ptr` [B, gw*gh + 1] i32 and `cell_kp` [B, kp_cap] i32 are kept
    on the device; `build` refreshes them for new keypoints of the same shape."""

    def __init__(self, kp, n_kp, W, H, cell=32, *, stream=None):
        self.W, self.H, self.cell = int(W), int(H), int(cell)
        self.gw = -(-self.W // self.cell)
        self.gh = -(-self.H // self.cell)
        B, kp_cap, _ = kp.shape
        self.cell_ptr = torch.zeros((B, self.gw * self.gh + 1), dtype=torch.int32, device=kp.device)
        self.cell_kp = torch.zeros((B, max(kp_cap, 1)), dtype=torch.int32, device=kp.device)
        self.build(kp, n_kp, stream=stream)

    def build(self, kp, n_kp, *, stream=None):
        B, kp_cap, _ = kp.shape
        if B != self.cell_ptr.shape[0] or kp_cap > self.cell_kp.shape[1]:
            raise ValueError("KeypointGrid.build: keypoint tensor of another shape")
        _lib.call("slam_kp_grid", ptr(kp), ptr(n_kp), kp_cap, B, self.W, self.H, self.cell,
                  ptr(self.cell_ptr), ptr(self.cell_kp), stream_ptr(stream))
        self.kp_cap = kp_cap
        return self


def window_knn2_batch(q, quv, qr, nq, t, kp, nt, grid: KeypointGrid, *, max_dist=64,
                      ratio=(7, 10), out=None, stream=None):
    """kNN-2 of every query among the keypoints inside its window
    (slam_hamming_window_knn2).

    q [q_cap,32] u8 (one query set shared by the batch) or [B,q_cap,32], quv
    [B,q_cap,2] f32 window centres, qr [B,q_cap] f32 half-sizes, nq [B] i32;
    t [B,t_cap,32] u8, kp [B,t_cap,5] f32, nt [B] i32 and the `grid` built from
    the same kp.  Returns (idx2, dist2 [B,q_cap,2] i32, good [B,q_cap] u8):
    good iff the best candidate is within max_dist and passes ratio[0]/ratio[1]
    against the second, when there is one.  Rows >= nq[b] are left untouched
    (-1 / 0 when allocated here)."""
    B, t_cap, _ = t.shape
    shared = q.dim() == 2
    q_cap = int(q.shape[-2])
    if grid.kp_cap != t_cap or grid.cell_ptr.shape[0] != B:
        raise ValueError("window_knn2_batch: the grid was built for other keypoints")
    if out is None:
        idx2 = torch.full((B, q_cap, 2), -1, dtype=torch.int32, device=t.device)
        dist2 = torch.full((B, q_cap, 2), -1, dtype=torch.int32, device=t.device)
        good = torch.zeros((B, q_cap), dtype=torch.uint8, device=t.device)
    else:
        idx2, dist2, good = out
    _lib.call("slam_hamming_window_knn2", ptr(q), int(shared), ptr(quv), ptr(qr), ptr(nq), q_cap,
              ptr(t), ptr(kp), ptr(nt), t_cap, ptr(grid.cell_ptr), ptr(grid.cell_kp), grid.W,
              grid.H, grid.cell, B, int(max_dist), int(ratio[0]), int(ratio[1]), ptr(idx2),
              ptr(dist2), ptr(good), stream_ptr(stream))
    return idx2, dist2, good


def unique_matches(idx2, dist2, good, nq, t_cap, *, out=None, stream=None):
    """Every keypoint to at most one query (slam_match_unique): the good query
    with the smallest (distance, index) keeps it.  Returns (owner [B,t_cap] i32,
    the winning query or -1; good' [B,q_cap] u8 with the losers cleared)."""
    B, q_cap = good.shape
    if out is None:
        owner = torch.full((B, max(t_cap, 1)), -1, dtype=torch.int32, device=good.device)
        good_out = torch.zeros((B, q_cap), dtype=torch.uint8, device=good.device)
    else:
        owner, good_out = out
    _lib.call("slam_match_unique", ptr(idx2), ptr(dist2), ptr(good), ptr(nq), q_cap, int(t_cap), B,
              ptr(owner), ptr(good_out), stream_ptr(stream))
    return owner, good_out


MAP_KNN_SEGMENT = int(_lib.lib.slam_hamming_map_segment())  # landmarks per workgroup of map_knn2_batch


def map_knn2_workspace(B, q_cap, x_cap, dev="cuda"):
    """The partial top-2 workspace of map_knn2_batch (u8; 8 bytes per item,
    segment of MAP_KNN_SEGMENT landmarks and query)."""
    nb = ctypes.c_size_t(0)
    _lib.call("slam_hamming_map_workspace_bytes", int(B), int(q_cap), int(x_cap), ctypes.byref(nb))
    return torch.empty(int(nb.value), dtype=torch.uint8, device=dev)


def map_knn2_batch(q, nq, desc, X, last, n, rng, *, max_dist=64, ratio=(7, 10), ws=None, out=None,
                   stream=None):
    """kNN-2 of keypoints against the live landmarks of one map, no window
    (slam_hamming_map_knn2).

    q [B,q_cap,32] u8, nq [B] i32; the map shared by the batch: desc [x_cap,32]
    u8, X [x_cap,3] f64, last [x_cap] i32 and the device count n [1] i32; rng
    [B,2] i32 (lo, hi) per item.  A landmark is eligible iff it lies below n, is
    alive (X[i,0] not NaN) and lo <= last[i] < hi.  Returns (idx2, dist2
    [B,q_cap,2] i32 with full landmark indices, good [B,q_cap] u8): good iff two
    candidates exist, the best is within max_dist and passes ratio[0]/ratio[1]
    against the second.  Rows >= nq[b] are left untouched (-1 / 0 when allocated
    here).  ws: map_knn2_workspace(B, q_cap, x_cap), the caller's for calls that
    may overlap; without one a buffer is allocated for this call."""
    B, q_cap, _ = q.shape
    x_cap = int(desc.shape[0])
    if out is None:
        idx2 = torch.full((B, q_cap, 2), -1, dtype=torch.int32, device=q.device)
        dist2 = torch.full((B, q_cap, 2), -1, dtype=torch.int32, device=q.device)
        good = torch.zeros((B, q_cap), dtype=torch.uint8, device=q.device)
    else:
        idx2, dist2, good = out
    if ws is None:
        ws = map_knn2_workspace(B, q_cap, x_cap, q.device)
        if stream is not None and stream != torch.cuda.current_stream(q.device):
            ws.record_stream(stream)
    _lib.call("slam_hamming_map_knn2", ptr(q), ptr(nq), q_cap, ptr(desc), ptr(X), ptr(last), ptr(n),
              x_cap, ptr(rng), B, int(max_dist), int(ratio[0]), int(ratio[1]), ptr(idx2), ptr(dist2),
              ptr(good), ptr(ws), ws.numel(), stream_ptr(stream))
    return idx2, dist2, good


def track_rows(idx2, good, nq, kp, frame0, *, out=None, stream=None):
    """The matches as [frame0 + b, query index, x, y] f64 rows in query order
    (slam_track_rows; the row format of MapStore.append) -> (rows [B,cap,4],
    count [B] i32), cap = min(q_cap, kp_cap)."""
    B, q_cap = good.shape
    kp_cap = int(kp.shape[1])
    if out is None:
        rows = torch.zeros((B, max(min(q_cap, kp_cap), 1), 4), dtype=torch.float64,
                           device=good.device)
        count = torch.zeros((B,), dtype=torch.int32, device=good.device)
    else:
        rows, count = out
    _lib.call("slam_track_rows", ptr(idx2), ptr(good), ptr(nq), q_cap, ptr(kp), kp_cap, B,
              int(frame0), int(rows.shape[1]), ptr(rows), ptr(count), stream_ptr(stream))
    return rows, count


def knn2(des_q, des_t):
    """Single (query, train) pair from host/device arrays -> numpy (idx2, dist2, good)."""
    require_gpu()
    des_q = np.ascontiguousarray(des_q if not isinstance(des_q, torch.Tensor)
                                 else des_q.cpu().numpy(), dtype=np.uint8).reshape(-1, 32)
    des_t = np.ascontiguousarray(des_t if not isinstance(des_t, torch.Tensor)
                                 else des_t.cpu().numpy(), dtype=np.uint8).reshape(-1, 32)
    nq, nt = des_q.shape[0], des_t.shape[0]
    q = to_dev(des_q.reshape(1, nq, 32) if nq else np.zeros((1, 1, 32), np.uint8))
    t = to_dev(des_t.reshape(1, nt, 32) if nt else np.zeros((1, 1, 32), np.uint8))
    nq_d = to_dev(np.array([nq], np.int32))
    nt_d = to_dev(np.array([nt], np.int32))
    idx2, dist2, good = knn2_batch(q, nq_d, t, nt_d)
    return (idx2[0, :nq].cpu().numpy(), dist2[0, :nq].cpu().numpy(),
            good[0, :nq].cpu().numpy().astype(bool))
