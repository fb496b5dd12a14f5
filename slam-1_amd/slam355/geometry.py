"""Device wrappers for gather / triangulation / PnP (csrc/geometry.hip)."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .device import ptr, require_gpu, stream_ptr

PNP_DEFAULTS = dict(n_hyp=100, reproj_thresh=8.0, hyp_iters=10, refine_iters=20)


def gather_matches(kpq, kpt, pairs, count, desq=None, dest=None, out=None, stream=None):
    """kp [B,cap,5] f32 + pairs [B,p_cap,2] -> (ptq, ptt [B,p_cap,2] f64, dq, dt [B,p_cap,32])."""
    B, p_cap, _ = pairs.shape
    dev = pairs.device
    if out is None:
        ptq = torch.zeros((B, p_cap, 2), dtype=torch.float64, device=dev)
        ptt = torch.zeros((B, p_cap, 2), dtype=torch.float64, device=dev)
        dq = dt = None
        if desq is not None:
            dq = torch.zeros((B, p_cap, 32), dtype=torch.uint8, device=dev)
            dt = torch.zeros((B, p_cap, 32), dtype=torch.uint8, device=dev)
    else:
        ptq, ptt, dq, dt = out
    _lib.call("slam_gather_matches", ptr(kpq), kpq.shape[1], ptr(kpt), kpt.shape[1], ptr(desq),
              ptr(dest), ptr(pairs), ptr(count), p_cap, B, ptr(ptq), ptr(ptt), ptr(dq), ptr(dt),
              stream_ptr(stream))
    return ptq, ptt, dq, dt


def gather_temporal(X, ptl, kp_next, pairs, count, out=None, stream=None):
    """-> (Q1 [B,p,3], q2 [B,p,2], q1 [B,p,2]) f64 (Point3D.py:50-52)."""
    B, pcap, _ = pairs.shape
    dev = pairs.device
    if out is None:
        Q1 = torch.zeros((B, pcap, 3), dtype=torch.float64, device=dev)
        q2 = torch.zeros((B, pcap, 2), dtype=torch.float64, device=dev)
        q1 = torch.zeros((B, pcap, 2), dtype=torch.float64, device=dev)
    else:
        Q1, q2, q1 = out
    _lib.call("slam_gather_temporal", ptr(X), ptr(ptl), X.shape[1], ptr(kp_next), kp_next.shape[1],
              ptr(pairs), ptr(count), pcap, B, ptr(Q1), ptr(q2), ptr(q1), stream_ptr(stream))
    return Q1, q2, q1


def fundamental_lmeds(m1, m2, count, seed=0, item0=0, n_hyp=300, out=None, stream=None, ws=None):
    """m1/m2 [B,cap,2] f64 -> (mask [B,cap] u8, F [B,9] f64, ninliers [B] i32).

    ws: the candidate workspace (fundamental_workspace(B, n_hyp)); calls that may
    run concurrently (other streams) must each pass their own.  Without one, the
    library takes a stream-ordered buffer for this call."""
    B, cap, _ = m1.shape
    dev = m1.device
    if out is None:
        mask = torch.zeros((B, max(cap, 1)), dtype=torch.uint8, device=dev)
        F = torch.zeros((B, 9), dtype=torch.float64, device=dev)
        ninl = torch.zeros((B,), dtype=torch.int32, device=dev)
    else:
        mask, F, ninl = out
    args = (ptr(m1), ptr(m2), ptr(count), cap, B, int(seed) & ((1 << 64) - 1), int(item0),
            int(n_hyp), ptr(mask), ptr(F), ptr(ninl))
    if ws is None:
        _lib.call("slam_fundamental_lmeds", *args, stream_ptr(stream))
    else:
        _lib.call("slam_fundamental_lmeds_ws", *args, ptr(ws), ws.numel(), stream_ptr(stream))
    return mask, F, ninl


def fundamental_workspace(B, n_hyp=300, dev="cuda"):
    """Candidate workspace of slam_fundamental_lmeds_ws for B pairs (f64)."""
    n = int(_lib.lib.slam_fundamental_workspace_len(B, n_hyp))
    return torch.empty(max(n, 1), dtype=torch.float64, device=dev)


def filter_pairs(pairs, count, mask, out=None, stream=None):
    """Keep pairs[b][k] with mask[b][k] (order preserved) -> (pairs', count')."""
    B, cap, _ = pairs.shape
    if out is None:
        o = torch.empty_like(pairs)
        oc = torch.empty((B,), dtype=torch.int32, device=pairs.device)
    else:
        o, oc = out
    _lib.call("slam_filter_pairs", ptr(pairs), ptr(count), ptr(mask), cap, B, ptr(o), ptr(oc),
              stream_ptr(stream))
    return o, oc


def project_landmarks(X, nx, poses, P, W, H, margin=0.0, min_depth=0.1, out=None, stream=None):
    """World points into `B` frames (slam_project_landmarks, step 1 of guided matching).

    X [cap,3] f64 (one map shared by every frame) or [B,cap,3], nx [B] i32,
    poses [B,4,4] f64 camera-to-world, P 3x4 (device tensor [3,4] f64, or an
    array uploaded here) -> (uv [B,cap,2] f32, NaN where the point is not
    visible; z [B,cap] f64 camera depth).  Rows >= nx[b] are left untouched
    (NaN / 0 when allocated here)."""
    B = int(poses.shape[0])
    shared = X.dim() == 2
    cap = int(X.shape[-2])
    Pd = P if isinstance(P, torch.Tensor) else torch.as_tensor(np.asarray(P, np.float64),
                                                               device=X.device)
    if out is None:
        uv = torch.full((B, cap, 2), float("nan"), dtype=torch.float32, device=X.device)
        z = torch.zeros((B, cap), dtype=torch.float64, device=X.device)
    else:
        uv, z = out
    _lib.call("slam_project_landmarks", ptr(X), int(shared), ptr(nx), cap, B, ptr(poses), ptr(Pd),
              int(W), int(H), float(margin), float(min_depth), ptr(uv), ptr(z), stream_ptr(stream))
    return uv, z


REFINE_LOSSES = {"linear": 0, "huber": 1, "soft_l1": 2, "cauchy": 3}


def refine_pose(rows, count, X, n_x, poses, P, *, loss="huber", loss_scale=2.4477, gate=2.4477,
                rounds=4, iters=10, min_inliers=10, min_depth=0.1, out=None, stream=None):
    """Robust pose refinement from track rows (slam_pose_refine; motion-only BA).

    rows [B,rows_cap,4] f64 and count [B] i32 as track_rows / LandmarkMap.observe
    return them, X [cap,3] f64 the map with its first n_x rows in use, poses
    [B,4,4] f64 camera-to-world (predicted), P 3x4 -> (poses [B,4,4] f64, mask
    [B,rows_cap] u8, ninl [B] i32, status [B] i32, info [B,6,6] f64, cost [B]
    f64).  status 0 ok, 1 too few valid observations, 2 too few inliers (1, 2:
    the input pose comes back, ninl -1).  The defaults 2.4477 = sqrt(5.991) are
    the 95 % chi-square bound of 2 degrees of freedom at sigma = 1 px.  `out`:
    the six outputs preallocated (poses may not be the input tensor)."""
    B, rows_cap = int(rows.shape[0]), int(rows.shape[1])
    dev = rows.device
    if loss not in REFINE_LOSSES:
        raise ValueError(f"refine_pose: loss {loss!r} is not one of {sorted(REFINE_LOSSES)}")
    n_x = int(n_x)
    if tuple(rows.shape) != (B, rows_cap, 4) or tuple(poses.shape) != (B, 4, 4) or \
            int(count.shape[0]) != B:
        raise ValueError("refine_pose: rows [B,cap,4], count [B] and poses [B,4,4] do not agree")
    if X.dim() != 2 or int(X.shape[1]) != 3 or not 0 <= n_x <= int(X.shape[0]):
        raise ValueError("refine_pose: X must be [cap,3] with 0 <= n_x <= cap")
    Pd = P if isinstance(P, torch.Tensor) else torch.as_tensor(np.asarray(P, np.float64),
                                                               device=dev)
    if out is None:
        po = torch.zeros((B, 4, 4), dtype=torch.float64, device=dev)
        mask = torch.zeros((B, rows_cap), dtype=torch.uint8, device=dev)
        ninl = torch.zeros((B,), dtype=torch.int32, device=dev)
        status = torch.zeros((B,), dtype=torch.int32, device=dev)
        info = torch.zeros((B, 6, 6), dtype=torch.float64, device=dev)
        cost = torch.zeros((B,), dtype=torch.float64, device=dev)
    else:
        po, mask, ninl, status, info, cost = out
        if po.data_ptr() == poses.data_ptr():
            raise ValueError("refine_pose: the output poses may not alias the input")
    _lib.call("slam_pose_refine", ptr(rows), ptr(count), rows_cap, B, ptr(X), n_x, ptr(poses),
              ptr(Pd), REFINE_LOSSES[loss], float(loss_scale), float(gate), float(min_depth),
              int(rounds), int(iters), int(min_inliers), ptr(po), ptr(mask), ptr(ninl), ptr(status),
              ptr(info), ptr(cost), stream_ptr(stream))
    return po, mask, ninl, status, info, cost


def points_workspace(n_frames, x_cap, dev="cuda"):
    """The index workspace of slam_points_refine for a window of n_frames (u8 tensor)."""
    nb = ctypes.c_size_t(0)
    _lib.call("slam_points_refine_workspace_bytes", int(n_frames), int(x_cap), ctypes.byref(nb))
    return torch.empty(max(int(nb.value), 4), dtype=torch.uint8, device=dev)


def refine_points(rows, count, poses, P, X, n_dev, *, loss="huber", loss_scale=2.4477, gate=2.4477,
                  min_depth=0.1, n_rounds=3, iters=8, min_obs=3, max_var=0.25, kill=False, out=None,
                  workspace=None, stream=None):
    """Structure-only refinement of the landmarks from track rows
    (slam_points_refine): the poses are held, every landmark is refined from all
    of its observations in the window, X is updated in place.

    rows [F,rows_cap,4] f64 and count [F] i32 as track_rows / LandmarkMap.observe
    and spawn leave them (the position in the window names the frame), poses
    [F,4,4] f64 camera-to-world, P 3x4, X [cap,3] f64, n_dev int32 [1] (device)
    the landmark count -> (status [cap] i32, nobs [cap] i32, cost [cap] f64, info
    [cap,3,3] f64, var [cap] f64, mask [F,rows_cap] u8, nkilled [1] i32).  status
    0 refined, 1 too few valid observations, 2 too few inliers, 3 the guard (a
    pivot of the information not positive, or its largest variance above max_var
    m^2 per px^2), 4 dead, -1 beyond the count; only status 0 moves the point.
    kill=True turns the status-2 landmarks dead (NaN) and counts them in nkilled,
    which is not written otherwise.  `out`: the seven outputs preallocated;
    `workspace`: points_workspace(F, cap).  With both given the call allocates
    nothing and can be captured in a graph."""
    F, rows_cap = int(rows.shape[0]), int(rows.shape[1])
    dev = rows.device
    if loss not in REFINE_LOSSES:
        raise ValueError(f"refine_points: loss {loss!r} is not one of {sorted(REFINE_LOSSES)}")
    if tuple(rows.shape) != (F, rows_cap, 4) or tuple(poses.shape) != (F, 4, 4) or \
            tuple(count.shape) != (F,):
        raise ValueError("refine_points: rows [F,cap,4], count [F] and poses [F,4,4] do not agree")
    if X.dim() != 2 or int(X.shape[1]) != 3 or not X.is_contiguous() or X.dtype != torch.float64:
        raise ValueError("refine_points: X must be a contiguous [cap,3] f64 tensor")
    if rows.dtype != torch.float64 or poses.dtype != torch.float64 or count.dtype != torch.int32 or \
            n_dev.dtype != torch.int32 or n_dev.numel() != 1:
        raise ValueError("refine_points: rows, poses f64; count, n_dev (one element) i32")
    if not (rows.is_contiguous() and poses.is_contiguous() and count.is_contiguous()):
        raise ValueError("refine_points: rows, count and poses must be contiguous")
    cap = int(X.shape[0])
    Pd = P if isinstance(P, torch.Tensor) else torch.as_tensor(np.asarray(P, np.float64),
                                                               device=dev)
    if out is None:
        out = (torch.zeros((cap,), dtype=torch.int32, device=dev),
               torch.zeros((cap,), dtype=torch.int32, device=dev),
               torch.zeros((cap,), dtype=torch.float64, device=dev),
               torch.zeros((cap, 3, 3), dtype=torch.float64, device=dev),
               torch.zeros((cap,), dtype=torch.float64, device=dev),
               torch.zeros((F, rows_cap), dtype=torch.uint8, device=dev),
               torch.zeros((1,), dtype=torch.int32, device=dev))
    status, nobs, cost, info, var, mask, nkilled = out
    if tuple(status.shape) != (cap,) or tuple(nobs.shape) != (cap,) or tuple(cost.shape) != (cap,) or \
            tuple(info.shape) != (cap, 3, 3) or tuple(var.shape) != (cap,) or \
            tuple(mask.shape) != (F, rows_cap) or nkilled.numel() != 1:
        raise ValueError("refine_points: out does not match (cap, F, rows_cap)")
    ws = workspace if workspace is not None else points_workspace(F, cap, dev)
    _lib.call("slam_points_refine", ptr(rows), ptr(count), rows_cap, F, ptr(poses), ptr(Pd), ptr(X),
              ptr(n_dev), cap, REFINE_LOSSES[loss], float(loss_scale), float(gate), float(min_depth),
              int(n_rounds), int(iters), int(min_obs), float(max_var), int(bool(kill)), ptr(status),
              ptr(nobs), ptr(cost), ptr(info), ptr(var), ptr(mask), ptr(nkilled), ptr(ws),
              ws.numel(), stream_ptr(stream))
    return status, nobs, cost, info, var, mask, nkilled


def triangulate(ptl, ptr_, count, P_l, P_r, out=None, stream=None):
    """ptl/ptr [B,cap,2] f64, P 3x4 (shared) or [B,3,4] -> X [B,cap,3] f64."""
    B, cap, _ = ptl.shape
    Pl = P_l if isinstance(P_l, torch.Tensor) else torch.as_tensor(np.asarray(P_l, np.float64),
                                                                   device=ptl.device)
    Pr = P_r if isinstance(P_r, torch.Tensor) else torch.as_tensor(np.asarray(P_r, np.float64),
                                                                   device=ptl.device)
    Pl, Pr = Pl.contiguous(), Pr.contiguous()
    stride = 12 if Pl.dim() == 3 else 0
    X = out if out is not None else torch.zeros((B, cap, 3), dtype=torch.float64, device=ptl.device)
    _lib.call("slam_triangulate", ptr(ptl), ptr(ptr_), ptr(count), cap, B, ptr(Pl), ptr(Pr), stride,
              ptr(X), stream_ptr(stream))
    return X


def pnp_ransac(Q, q, count, K, seed=0, item0=0, out=None, stream=None, ws=None, scratch=None,
               **kw):
    """Q [B,cap,3], q [B,cap,2] f64 -> (rvec [B,3], tvec [B,3], ninliers [B], mask [B,cap]).

    ws: the hypothesis-pose workspace (pnp_workspace(B, n_hyp)); calls that may
    run concurrently (other streams) must each pass their own.  Without one, a
    fresh buffer is allocated for this call (and kept alive for `stream`).
    scratch: the EPnP scratch (pnp_scratch(B, n_hyp)), the caller's in the same
    way.  Without one, the library takes a stream-ordered buffer for this call."""
    prm = dict(PNP_DEFAULTS, **kw)
    B, cap, _ = Q.shape
    dev = Q.device
    Kt = K if isinstance(K, torch.Tensor) else torch.as_tensor(np.asarray(K, np.float64), device=dev)
    if out is None:
        rvec = torch.zeros((B, 3), dtype=torch.float64, device=dev)
        tvec = torch.zeros((B, 3), dtype=torch.float64, device=dev)
        ninl = torch.zeros((B,), dtype=torch.int32, device=dev)
        mask = torch.zeros((B, max(cap, 1)), dtype=torch.uint8, device=dev)
    else:
        rvec, tvec, ninl, mask = out
    if ws is None:
        ws = pnp_workspace(B, prm["n_hyp"], dev)
        if stream is not None and stream != torch.cuda.current_stream(dev):
            ws.record_stream(stream)  # freed by the caching allocator only after `stream`
    args = (ptr(Q), ptr(q), ptr(count), cap, B, ptr(Kt.contiguous()),
            int(seed) & ((1 << 64) - 1), int(item0), prm["n_hyp"], float(prm["reproj_thresh"]),
            prm["hyp_iters"], prm["refine_iters"], ptr(rvec), ptr(tvec), ptr(ninl), ptr(mask),
            ptr(ws), ws.numel())
    if scratch is None:
        _lib.call("slam_pnp_ransac", *args, stream_ptr(stream))
    else:
        _lib.call("slam_pnp_ransac_ws", *args, ptr(scratch), scratch.numel(), stream_ptr(stream))
    return rvec, tvec, ninl, mask


def pnp_workspace(B, n_hyp=PNP_DEFAULTS["n_hyp"], dev="cuda"):
    """Hypothesis-pose workspace of slam_pnp_ransac for B items (f64)."""
    n = int(_lib.lib.slam_pnp_workspace_len(B, n_hyp))
    return torch.empty(max(n, 1), dtype=torch.float64, device=dev)


def pnp_scratch(B, n_hyp=PNP_DEFAULTS["n_hyp"], dev="cuda"):
    """EPnP scratch of slam_pnp_ransac_ws for B items (f64)."""
    n = int(_lib.lib.slam_pnp_scratch_len(B, n_hyp))
    return torch.empty(max(n, 1), dtype=torch.float64, device=dev)


VO_DEFAULTS = dict(max_iter=100, lm_iters=20, early_stop=5)


def vo_estimate_pose(q1, q2, Q1, Q2, count, P, seed=0, item0=0, out=None, stream=None, **kw):
    """visual_odometry.py:135-157 batched: q1, q2 [B,cap,2], Q1, Q2 [B,cap,3] f64,
    P 3x4 -> (pose [B,6] (rotvec, t), best [B], ntried [B], err [B])."""
    prm = dict(VO_DEFAULTS, **kw)
    B, cap, _ = Q1.shape
    dev = Q1.device
    Pt = P if isinstance(P, torch.Tensor) else torch.as_tensor(np.asarray(P, np.float64), device=dev)
    if out is None:
        pose = torch.zeros((B, 6), dtype=torch.float64, device=dev)
        best = torch.zeros((B,), dtype=torch.int32, device=dev)
        ntried = torch.zeros((B,), dtype=torch.int32, device=dev)
        err = torch.zeros((B,), dtype=torch.float64, device=dev)
    else:
        pose, best, ntried, err = out
    nb = ctypes.c_size_t(0)
    _lib.call("slam_vo_pose_workspace_bytes", B, prm["max_iter"], ctypes.byref(nb))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    _lib.call("slam_vo_estimate_pose", ptr(q1), ptr(q2), ptr(Q1), ptr(Q2), ptr(count), cap, B,
              ptr(Pt.contiguous()), int(seed) & ((1 << 64) - 1), int(item0), prm["max_iter"],
              prm["lm_iters"], prm["early_stop"], ptr(pose), ptr(best), ptr(ntried), ptr(err),
              ptr(ws), nb.value, stream_ptr(stream))
    return pose, best, ntried, err


def vo_residuals(dof, q1, q2, Q1, Q2, count, P, out=None, stream=None):
    """visual_odometry.py:65-81 batched: dof [B,6] -> f [B, 4 cap] (first 4 count[b] valid)."""
    B, cap, _ = Q1.shape
    dev = Q1.device
    Pt = P if isinstance(P, torch.Tensor) else torch.as_tensor(np.asarray(P, np.float64), device=dev)
    f = out if out is not None else torch.zeros((B, 4 * max(cap, 1)), dtype=torch.float64,
                                                device=dev)
    _lib.call("slam_vo_residuals", ptr(dof), ptr(q1), ptr(q2), ptr(Q1), ptr(Q2), ptr(count), cap,
              B, ptr(Pt.contiguous()), ptr(f), stream_ptr(stream))
    return f
