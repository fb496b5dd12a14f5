"""Pose-chain (loop-closure) optimisation on the GPU — host side of
csrc/posegraph.hip.

The reference's live bundle adjustment (/root/reference/BundleAdjustment.py:
79-225) optimises m relative poses [r0 r1 r2 t0 t1 t2] so that the weighted
per-frame motion costs stay small and the chained absolute pose closes the
loop (end pose = start pose), with scipy's TRF.  Here:
  chain_objective(params, loop)  batched objective / objective_without_loop_
                                 closure (one launch for any number of vectors)
  PoseChain                      device-resident TRF (x_scale='jac', exact
                                 trust-region subproblem, analytic Jacobian)
The drop-in names live in slam355.BundleAdjustment.

The general SE(3) pose graph (csrc/posegraph_se3.hip) is beside
it: weighted relative-pose edges between arbitrary keyframes, LM on the device
over a skyline tile Cholesky:
  PoseGraph                      the device-resident graph and its LM; covariance /
                                 relative_covariance / gate
  pg_schedule                    the host-built schedule of the skyline factor
  pg_cov_plan                    the tile columns a covariance request costs
  relative_pose                  the measurement an edge stores
  edges_from_ba                  weighted edges from a refined BA window
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .device import ptr, require_gpu, stream_ptr

STATUS = {0: "max_nfev", 1: "gtol", 2: "ftol", 3: "xtol", 4: "ftol+xtol"}


def chain_objective(params, loop: bool = True) -> np.ndarray:
    """objective (loop=True: m + 2 residuals) or objective_without_loop_closure
    (m residuals) of one [6m] or a batch [B, 6m] of parameter vectors."""
    dev = require_gpu()
    p = np.asarray(params, np.float64)
    single = p.ndim == 1
    p = np.atleast_2d(p)
    if p.shape[1] % 6:
        raise ValueError("car_params must hold 6 values per frame")
    B, m = p.shape[0], p.shape[1] // 6
    nr = m + (2 if loop else 0)
    tp = torch.from_numpy(np.ascontiguousarray(p)).to(dev)
    out = torch.empty((B, nr), dtype=torch.float64, device=dev)
    _lib.call("slam_pose_chain_objective", ptr(tp), B, m, int(loop), ptr(out), stream_ptr())
    r = out.cpu().numpy()
    return r[0] if single else r


class PoseChain:
    """Device-resident TRF run over m relative poses (scipy least_squares
    method='trf', x_scale='jac' semantics: ftol / xtol / gtol tests, max_nfev,
    trust-radius rules, the 'exact' subproblem)."""

    def __init__(self, car_params, loop: bool = True, stream=None):
        dev = require_gpu()
        x = np.ascontiguousarray(np.asarray(car_params, np.float64).ravel())
        if x.size == 0 or x.size % 6:
            raise ValueError("car_params must hold 6 values per frame (and at least one frame)")
        self.m, self.loop, self.stream = x.size // 6, bool(loop), stream
        n = int(_lib.lib.slam_pose_chain_workspace_len(self.m))
        self.ws = torch.zeros(n, dtype=torch.float64, device=dev)
        self.ws[: x.size].copy_(torch.from_numpy(x))
        self.st = torch.zeros(16, dtype=torch.float64, device=dev)
        self._started = False

    def run(self, max_iter: int, ftol=1e-8, xtol=1e-8, gtol=1e-8, max_nfev=None):
        """Up to max_iter outer TRF iterations (resumes a previous run)."""
        max_nfev = 100 * 6 * self.m if max_nfev is None else int(max_nfev)
        _lib.call("slam_pose_chain_trf", ptr(self.ws), self.m, int(self.loop), int(max_iter),
                  int(not self._started), float(ftol), float(xtol), float(gtol), max_nfev,
                  ptr(self.st), stream_ptr(self.stream))
        self._started = True

    def solve(self, ftol=1e-8, xtol=1e-8, gtol=1e-8, max_nfev=None, chunk=64) -> dict:
        """Iterate until a termination test fires or max_nfev (host checks the
        status between chunks of `chunk` iterations)."""
        max_nfev = 100 * 6 * self.m if max_nfev is None else int(max_nfev)
        while True:
            self.run(chunk, ftol, xtol, gtol, max_nfev)
            s = self.state()
            if s["status"] != 0 or s["nfev"] >= max_nfev:
                return s

    def state(self) -> dict:
        s = self.st.cpu().numpy()
        return dict(cost0=float(s[0]), cost=float(s[1]), nfev=int(s[2]), njev=int(s[3]),
                    status=int(s[4]), message=STATUS[int(s[4])], Delta=float(s[5]),
                    alpha=float(s[6]), iterations=int(s[7]))

    def params(self) -> np.ndarray:
        return self.ws[: 6 * self.m].cpu().numpy().copy()


# ----------------------------------------------------------------------------- SE(3) pose graph
PG_MAGIC = 0x50473031
PG_HDR = 16
PG_TILE_POSES = 10  # poses per 64x64 tile (60 rows, 4 of padding)
ST = dict(LAMBDA=0, NU=1, COST=2, COST_NEW=3, PRED=4, RHO=5, ACCEPTED=6, CUR=7, ITERS=8, NACCEPT=9,
          CHOL_FAIL=11)  # SLAM_BA_ST_*
FIXED_POSE = 0x3F


def _check_edges(n_poses, edges):
    e = np.asarray(edges)
    if e.ndim != 2 or e.shape[1] != 2 or len(e) == 0 or not np.issubdtype(e.dtype, np.integer):
        raise ValueError("edges must be a non-empty integer array [E, 2]")
    if n_poses < 1 or e.min() < 0 or e.max() >= n_poses:
        raise ValueError("edge index outside [0, n_poses)")
    if np.any(e[:, 0] == e[:, 1]):
        raise ValueError("an edge joins a pose to itself")
    return np.ascontiguousarray(e, np.int32)


def pg_tables(n_poses, edges, full=False):
    """The tables of the skyline schedule as a dict (pg_schedule packs them):
    first[T], rowoff[T + 1], pose_ptr / pose_ent (pose -> 2 edge + side, edge
    order), pair_ptr / pair_ij / pair_ent (sorted unique (lo, hi) -> 2 edge +
    (i > j), edge order), col_ptr / rows (panel rows {I > k : first[I] <= k}
    of column k, ascending), upd_ptr / upd (its update pairs (I, J), I >= J,
    over those rows).  Tiles hold PG_TILE_POSES poses in keyframe order; tile
    row I stores the columns first[I]..I.  full: first[I] = 0 (the dense lower
    triangle, for comparison)."""
    e = _check_edges(n_poses, edges)
    N, E = int(n_poses), len(e)
    T = (N + PG_TILE_POSES - 1) // PG_TILE_POSES
    lo, hi = e.min(1), e.max(1)
    first = np.arange(T, dtype=np.int64)
    if full:
        first[:] = 0
    else:
        np.minimum.at(first, hi // PG_TILE_POSES, lo // PG_TILE_POSES)
    rowoff = np.concatenate([[0], np.cumsum(np.arange(T) - first + 1)])
    # pose -> (edge, side): a stable sort of the 2 E entries by pose keeps edge order
    ent = np.arange(2 * E)
    order = np.argsort(e.ravel(), kind="stable")
    pose_ptr = np.concatenate([[0], np.cumsum(np.bincount(e.ravel(), minlength=N))])
    pose_ent = ent[order]
    key = lo.astype(np.int64) * N + hi
    uk, inv = np.unique(key, return_inverse=True)
    P = len(uk)
    porder = np.argsort(inv, kind="stable")
    pair_ptr = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=P))])
    pair_ij = np.stack([uk // N, uk % N], 1)
    pair_ent = 2 * porder + (e[porder, 0] > e[porder, 1])
    col_ptr, upd_ptr, rows, upd = [0], [0], [], []
    for k in range(T):
        rk = [I for I in range(k + 1, T) if first[I] <= k]
        rows += rk
        upd += [(I, J) for a, I in enumerate(rk) for J in rk[: a + 1]]
        col_ptr.append(len(rows))
        upd_ptr.append(len(upd))
    i32 = lambda a: np.asarray(a, np.int32).reshape(-1)  # noqa: E731
    return dict(N=N, E=E, T=T, P=P, n_tiles=int(rowoff[-1]), first=i32(first), rowoff=i32(rowoff),
                pose_ptr=i32(pose_ptr), pose_ent=i32(pose_ent), pair_ptr=i32(pair_ptr),
                pair_ij=i32(pair_ij), pair_ent=i32(pair_ent), col_ptr=i32(col_ptr), upd_ptr=i32(upd_ptr),
                rows=i32(rows), upd=i32(upd))


def pg_schedule(n_poses, edges, full=False):
    """The int32 schedule of slam_pg_problem.sched (layout: include/slam355.h)."""
    t = pg_tables(n_poses, edges, full)
    m = np.diff(t["col_ptr"])
    hdr = np.zeros(PG_HDR, np.int32)
    hdr[:10] = [PG_MAGIC, t["N"], t["E"], t["T"], t["P"], t["n_tiles"], len(t["rows"]), len(t["upd"]) // 2,
                m.max(initial=0), (m * (m + 1) // 2).max(initial=0)]
    return np.concatenate([hdr] + [t[k] for k in ("first", "rowoff", "pose_ptr", "pose_ent", "pair_ptr", "pair_ij",
                                                  "pair_ent", "col_ptr", "upd_ptr", "rows", "upd")])


# host SO(3) helpers (edges_from_ba's propagation; the device code has its own)
def _hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _so3_exp(r):
    t2 = float(r @ r)
    th = np.sqrt(t2)
    a = 1.0 - t2 / 6.0 if th < 1e-4 else np.sin(th) / th
    b = 0.5 - t2 / 24.0 if th < 1e-4 else 2.0 * np.sin(0.5 * th) ** 2 / t2
    K = _hat(r)
    return np.eye(3) + a * K + b * (K @ K)


def _so3_jr(r):
    t2 = float(r @ r)
    th = np.sqrt(t2)
    b = 0.5 - t2 / 24.0 if th < 1e-4 else 2.0 * np.sin(0.5 * th) ** 2 / t2
    c = 1.0 / 6.0 - t2 / 120.0 if th < 1e-4 else (th - np.sin(th)) / (t2 * th)
    K = _hat(r)
    return np.eye(3) - b * K + c * (K @ K)


def _so3_jr_inv(r):
    t2 = float(r @ r)
    th = np.sqrt(t2)
    k = 1.0 / 12.0 + t2 / 720.0 if th < 1e-4 else (1.0 - 0.5 * th / np.tan(0.5 * th)) / t2
    K = _hat(r)
    return np.eye(3) + 0.5 * K + k * (K @ K)


def _so3_log(R):
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = np.linalg.norm(v), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, c)
    if c < 0.0 and s < 1e-3:  # at pi: the axis from the symmetric part
        w, V = np.linalg.eigh(0.5 * (R + R.T))
        n = V[:, -1]
        return th * (n if v @ n >= 0.0 else -n)
    return v * (1.0 + s * s / 6.0 if s < 1e-4 and c > 0 else th / s)


def relative_pose(x_i, x_j):
    """The 6-vector [r, t] of T_i^-1 T_j for poses x = [r (Rodrigues), t], T =
    [R(r) | t]: the measurement a PoseGraph edge (i, j) stores."""
    x_i, x_j = np.asarray(x_i, np.float64), np.asarray(x_j, np.float64)
    Ri = _so3_exp(x_i[:3])
    return np.concatenate([_so3_log(Ri.T @ _so3_exp(x_j[:3])), Ri.T @ (x_j[3:6] - x_i[3:6])])


def relative_pose_jacobian(x_i, x_j):
    """d relative_pose / d [x_i, x_j]: [6, 12] (the edge Jacobian at Z = I)."""
    x_i, x_j = np.asarray(x_i, np.float64), np.asarray(x_j, np.float64)
    Ri, Rj = _so3_exp(x_i[:3]), _so3_exp(x_j[:3])
    z = relative_pose(x_i, x_j)
    Jinv = _so3_jr_inv(z[:3])
    G = np.zeros((6, 12))
    G[:3, :3] = -Jinv @ Rj.T @ Ri @ _so3_jr(x_i[:3])
    G[:3, 6:9] = Jinv @ _so3_jr(x_j[:3])
    G[3:, :3] = _hat(z[3:]) @ _so3_jr(x_i[:3])
    G[3:, 3:6] = -Ri.T
    G[3:, 9:12] = Ri.T
    return G


def edges_from_ba(problem, pairs, scale="unit", rank_tol=1e-8):
    """Weighted pose-graph edges from a refined BA window: for each keyframe
    pair (a, b) of `pairs` [m, 2] of a BAProblem (or a BAWindowSet window) the
    measurement z = relative_pose(x_a, x_b) at the live cameras and its 6x6
    information matrix, the inverse of the first-order covariance G [Saa Sab;
    Sab^T Sbb] G^T with G = relative_pose_jacobian and the 6x6 pose blocks of
    problem.covariance(cameras, pairs, scale).

    Pose convention: an edge's poses are the BAL cameras' own [r, t], i.e.
    world -> camera (x_cam = R(r) X + t, T = [R | t]); no conversion is made,
    f, k1, k2 are marginalised by dropping their rows.  A PoseGraph over these
    edges therefore takes cams[:, :6] as its poses, and z is the transform
    camera b -> camera a composed as T_a^-1 T_b in that convention.
    Returns (edges int32 [m, 2], meas [m, 6], information [m, 6, 6]).  Raises
    np.linalg.LinAlgError where covariance() does, and when a propagated
    covariance is not positive definite (a pair of held cameras)."""
    pr = np.asarray(pairs)
    if pr.ndim != 2 or pr.shape[1] != 2 or len(pr) == 0:
        raise ValueError("pairs must be a non-empty [m, 2] list of keyframe pairs")
    if np.any(pr[:, 0] == pr[:, 1]):
        raise ValueError("a pair joins a keyframe to itself")
    cams = problem.params()[0]
    uniq = np.unique(pr)
    cov = problem.covariance(cameras=uniq, pairs=pr, scale=scale, rank_tol=rank_tol)
    own = {int(c): cov[q][:6, :6] for q, c in enumerate(uniq)}
    meas, info = np.zeros((len(pr), 6)), np.zeros((len(pr), 6, 6))
    for q, (a, b) in enumerate(pr):
        xa, xb = cams[a, :6], cams[b, :6]
        Sab = cov[len(uniq) + q][:6, :6]
        S = np.block([[own[int(a)], Sab], [Sab.T, own[int(b)]]])
        G = relative_pose_jacobian(xa, xb)
        Sz = G @ S @ G.T
        Sz = 0.5 * (Sz + Sz.T)
        np.linalg.cholesky(Sz)  # LinAlgError when not positive definite
        meas[q] = relative_pose(xa, xb)
        info[q] = np.linalg.inv(Sz)
    return np.ascontiguousarray(pr, np.int32), meas, info


def edge_from_localization(x_ref, pose_c2w, info, return_map=False):
    """A weighted PoseGraph edge (ref, current) from a pose localized against the
    map (LandmarkMap.localize / relocalize): the measurement and information in
    the world -> camera convention of edges_from_ba.

    pose_c2w [4,4] camera-to-world [R | t]; info [6,6] the information of the
    perturbation X_cam <- Exp(dw) X_cam + dv in the order (dw, dv), as
    slam_pose_refine defines it; x_ref [6] the reference pose [r, t], world ->
    camera, treated as exact (its own uncertainty is the graph's).
      x_cur    = [log(R^T), -R^T t]
      S_pose   = M info^-1 M^T,  M = [[J_l^-1(r), 0], [-[t]x, I]] at x_cur
                 (the left perturbation in the coordinates [r, t])
      meas     = relative_pose(x_ref, x_cur)
      information = (G S_pose G^T)^-1,  G = the last six columns of
                 relative_pose_jacobian(x_ref, x_cur).
    Batched: B poses [B,4,4], info [B,6,6] and one x_ref per frame [B,6] ->
    ([B,6], [B,6,6]).  np.linalg.LinAlgError when info is not positive
    definite.  return_map: also the 6x6 map G M from (dw, dv) to the change of
    meas."""
    T = np.asarray(pose_c2w, np.float64)
    single = T.ndim == 2
    T = T.reshape(-1, 4, 4)
    B = len(T)
    A = np.asarray(info, np.float64).reshape(-1, 6, 6)
    xr = np.asarray(x_ref, np.float64).reshape(-1, 6)
    if len(A) != B or len(xr) != B:
        raise ValueError("edge_from_localization: one info and one x_ref per pose")
    if not (np.all(np.isfinite(T)) and np.all(np.isfinite(A)) and np.all(np.isfinite(xr))):
        raise ValueError("edge_from_localization: poses, info and x_ref must be finite")
    meas, information, maps = np.zeros((B, 6)), np.zeros((B, 6, 6)), np.zeros((B, 6, 6))
    for b in range(B):
        Rt = T[b, :3, :3].T
        x_cur = np.concatenate([_so3_log(Rt), -Rt @ T[b, :3, 3]])
        S = 0.5 * (A[b] + A[b].T)
        np.linalg.cholesky(S)  # LinAlgError when not positive definite
        M = np.eye(6)
        M[:3, :3] = _so3_jr_inv(-x_cur[:3])
        M[3:, :3] = -_hat(x_cur[3:])
        L = relative_pose_jacobian(xr[b], x_cur)[:, 6:] @ M
        Sz = L @ np.linalg.inv(S) @ L.T
        Sz = 0.5 * (Sz + Sz.T)
        np.linalg.cholesky(Sz)
        W = np.linalg.inv(Sz)
        meas[b], information[b], maps[b] = relative_pose(xr[b], x_cur), 0.5 * (W + W.T), L
    out = (meas[0], information[0], maps[0]) if single else (meas, information, maps)
    return out if return_map else out[:2]


CHI2_6_99 = 16.811893829770927  # the 0.99 quantile of chi^2 with 6 degrees of freedom


def _cov_list(n_poses, a, what, distinct=False):
    """`a` as a contiguous non-empty int32 [m, 2] list of pose indices."""
    a = np.asarray(a)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what} must be integer pose indices")
    if a.ndim != 2 or a.shape[1] != 2 or len(a) == 0:
        raise ValueError(f"{what} must be a non-empty [m, 2] list, not shape {list(a.shape)}")
    if int(n_poses) < 1 or a.min() < 0 or a.max() >= n_poses:
        raise ValueError(f"{what}: index outside [0, {n_poses})")
    if distinct and np.any(a[:, 0] == a[:, 1]):
        raise ValueError(f"{what}: an entry joins a pose to itself")
    return np.ascontiguousarray(a, np.int32)


def pg_cov_plan(n_poses, pairs, gate=False):
    """What a covariance request costs (slam_pg_covariance).
    Block (a, b) is read from the tile column of the larger index: `requests`
    [m, 2] holds (min, max) per entry, so a pair in either order is the same
    request; `cols` the distinct tile columns max // PG_TILE_POSES, ascending,
    each one 64-column solve through the factor; `low` the lowest tile row min
    // PG_TILE_POSES asked of each column (the backward sweep of a column
    stops there).  gate: the entries are candidate edges, which also need both
    poses' own blocks.  Pure NumPy; len(cols) sizes the workspace."""
    pr = _cov_list(n_poses, pairs, "pairs")
    req = np.stack([pr.min(1), pr.max(1)], 1)
    r, c = req[:, 0] // PG_TILE_POSES, req[:, 1] // PG_TILE_POSES
    if gate:
        r, c = np.concatenate([r, r]), np.concatenate([c, r])
    cols = np.unique(c)
    low = np.array([r[c == k].min() for k in cols], np.int32)
    return dict(requests=req.astype(np.int32), cols=cols.astype(np.int32), low=low)


def _rank_tol(rank_tol):
    rank_tol = float(rank_tol)
    if not (np.isfinite(rank_tol) and 0.0 <= rank_tol < 1.0):
        raise ValueError(f"rank_tol must be finite and in [0, 1), not {rank_tol!r}")
    return rank_tol


class PoseGraph:
    """A device-resident SE(3) pose graph and its Levenberg-Marquardt.

    poses [N, 6]: x_i = [r (Rodrigues vector), t], T_i = [R(r_i) | t_i].
    edges [E, 2], meas [E, 6]: edge k = (i, j) measures z_k = T_i^-1 T_j
    (relative_pose); i != j in either order, repeated pairs allowed.
    information [E, 6, 6] (factored here: the upper Cholesky factor A with A^T
    A = information; LinAlgError when one is not positive definite) or
    sqrt_information [E, 6, 6] = A directly; neither: identity.  fixed: None,
    or one word per pose (bit p holds parameter p, FIXED_POSE the pose whole),
    or a bool [N, 6].  The gauge is the caller's: hold one pose.  loss,
    f_scale: as BAProblem's, on s = |A_k e_k|^2 per edge."""

    def __init__(self, poses, edges, meas, information=None, sqrt_information=None, fixed=None,
                 loss="linear", f_scale=1.0, stream=None, lam0=1e-4, _full_profile=False):
        from .ba import loss_args

        dev = require_gpu()
        x = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 6))
        self.N = len(x)
        e = _check_edges(self.N, edges)
        self.E = len(e)
        z = np.ascontiguousarray(np.asarray(meas, np.float64).reshape(-1, 6))
        if len(z) != self.E:
            raise ValueError("meas must hold 6 values per edge")
        if information is not None and sqrt_information is not None:
            raise ValueError("give information or sqrt_information, not both")
        if information is not None:
            info = np.asarray(information, np.float64).reshape(self.E, 6, 6)
            A = np.stack([np.linalg.cholesky(m).T for m in info])
        elif sqrt_information is not None:
            A = np.asarray(sqrt_information, np.float64).reshape(self.E, 6, 6)
        else:
            A = np.tile(np.eye(6), (self.E, 1, 1))
        if not (np.all(np.isfinite(x)) and np.all(np.isfinite(z)) and np.all(np.isfinite(A))):
            raise ValueError("poses, meas and the information must be finite")
        code, scale = loss_args(loss, f_scale)
        words = None
        if fixed is not None:
            f = np.asarray(fixed)
            if f.dtype == bool:
                f = (f.reshape(self.N, 6).astype(np.uint32) << np.arange(6, dtype=np.uint32)).sum(1)
            if f.shape != (self.N,) or np.any(f < 0) or np.any(f > FIXED_POSE):
                raise ValueError("fixed: one word in [0, 0x3F] per pose, or a bool [N, 6]")
            words = np.ascontiguousarray(f, np.uint32)
        self.stream = stream
        self.edges = e
        self.sched_host = pg_schedule(self.N, e, full=_full_profile)  # kept alive: the library reads it
        self.n_tiles = int(self.sched_host[5])
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        n_ws = int(_lib.lib.slam_pg_workspace_len(self.N, self.E, self.n_tiles))
        self.t = dict(x0=T(x), x1=T(x), edges=T(e), meas=T(z), A=T(A), sched=T(self.sched_host),
                      ws=torch.zeros(n_ws, dtype=torch.float64, device=dev),
                      state=torch.zeros(20, dtype=torch.float64, device=dev))
        if words is not None:
            self.t["fixed"] = T(words)
        s = _lib.PGProblemStruct()
        s.n_poses, s.n_edges, s.loss, s.sched_len = self.N, self.E, code, len(self.sched_host)
        s.loss_scale = scale
        s.poses[0], s.poses[1] = self.t["x0"].data_ptr(), self.t["x1"].data_ptr()
        s.edge_ij, s.edge_ij_host = self.t["edges"].data_ptr(), self.edges.ctypes.data
        s.meas, s.sqrt_info = self.t["meas"].data_ptr(), self.t["A"].data_ptr()
        s.pose_fixed = self.t["fixed"].data_ptr() if words is not None else None
        s.sched, s.sched_host = self.t["sched"].data_ptr(), self.sched_host.ctypes.data
        s.ws, s.ws_len, s.state = self.t["ws"].data_ptr(), n_ws, self.t["state"].data_ptr()
        self._s = s
        self.reset(lam0)

    def _sp(self):
        return stream_ptr(self.stream)

    def reset(self, lam0=1e-4):
        """LM state <- (lam0, nu = 2), COST at the first buffer's poses."""
        _lib.call("slam_pg_reset", ctypes.byref(self._s), float(lam0), self._sp())

    def iterate(self, n: int = 1, lam0=None):
        """n LM iterations, no host synchronisation (lam0: reset first)."""
        if lam0 is not None:
            if self.state()["CUR"] != 0.0:
                self.t["x0"].copy_(self.t["x1"])
            self.reset(lam0)
        _lib.call("slam_pg_iterate", ctypes.byref(self._s), int(n), self._sp())

    def solve(self, max_iter=100, ftol=1e-10, xtol=1e-10, chunk=5) -> dict:
        """Iterate in chunks of `chunk` until a chunk that accepted a step
        lowered the cost by less than ftol (relative) or moved no parameter by
        more than xtol (1 + |x|), until lambda saturates, or max_iter."""
        done, st = 0, self.state()
        x = self.poses()
        while done < max_iter:
            k = min(chunk, max_iter - done)
            c0, n0 = st["COST"], st["NACCEPT"]
            self.iterate(k)
            done += k
            st, xn = self.state(), self.poses()
            if st["LAMBDA"] >= 1e30:
                break
            if st["NACCEPT"] > n0 and (abs(c0 - st["COST"]) <= ftol * max(st["COST"], 1e-300)
                                       or np.max(np.abs(xn - x) / (1.0 + np.abs(x))) <= xtol):
                break
            x = xn
        return st

    def state(self) -> dict:
        s = self.t["state"].cpu().numpy()
        return {k: float(s[v]) for k, v in ST.items()}

    def poses(self) -> np.ndarray:
        """[N, 6] at the live parameters."""
        cur = int(self.t["state"][ST["CUR"]].item() != 0)
        return self.t[f"x{cur}"].cpu().numpy().reshape(self.N, 6).copy()

    def residuals(self, weighted=True) -> np.ndarray:
        """[E, 6] at the live poses: sqrt(w) A e (weighted) or the raw e."""
        out = torch.empty((self.E, 6), dtype=torch.float64, device=self.t["state"].device)
        _lib.call("slam_pg_residual", ctypes.byref(self._s), None if weighted else ptr(out),
                  ptr(out) if weighted else None, self._sp())
        return out.cpu().numpy()

    def jacobian(self):
        """(J_i, J_j), [E, 6, 6] each: sqrt(w) A d e / d x_i, x_j, held columns zero."""
        dev = self.t["state"].device
        Ji = torch.empty((self.E, 6, 6), dtype=torch.float64, device=dev)
        Jj = torch.empty_like(Ji)
        _lib.call("slam_pg_jacobian", ctypes.byref(self._s), ptr(Ji), ptr(Jj), self._sp())
        return Ji.cpu().numpy(), Jj.cpu().numpy()

    # ------------------------------------------------------------------ covariance
    def _cov_ws(self, n_cols):
        """The covariance workspace for n_cols tile columns (grown on demand and
        kept) and the two status words."""
        n = int(_lib.lib.slam_pg_cov_workspace_len(self.N, int(n_cols)))
        if n < 0:
            raise _lib.SlamError(_lib.lib.slam_last_error().decode())
        dev = self.t["state"].device
        if getattr(self, "_cws", None) is None or self._cws.numel() < n:
            self._cws = None
            self._cws = torch.empty(n, dtype=torch.float64, device=dev)
        if getattr(self, "_cov_status", None) is None:
            self._cov_status = torch.zeros(2, dtype=torch.int32, device=dev)
        return self._cws

    def cov_status(self) -> int:
        """Status of the last covariance / gate call: 0 ok, 1 H0 not positive definite."""
        return int(self._cov_status[0].item())

    def gate_undetermined(self) -> int:
        """Candidates of the last gate / relative_covariance call whose d2 is NaN
        because their own S = P + R failed the rank test."""
        return int(self._cov_status[1].item())

    def _cov_raise(self, rank_tol):
        if self.cov_status() != 0:
            raise np.linalg.LinAlgError(
                "pose-graph covariance: J~^T J~ is not positive definite at "
                f"rank_tol {rank_tol:g} (fix the gauge: hold one pose whole)")

    def covariance(self, poses=None, pairs=None, rank_tol=1e-8, device=False):
        """Blocks of Sigma = (J~^T J~)^-1 at the live poses, zero damping, J~
        the Jacobian of the LM steps (robust and information weights, held
        columns out): [m, 6, 6] float64, Cov(x_a, x_a) per pose a of `poses`,
        then Cov(x_a, x_b) per (a, b) of `pairs` (None, None: every pose's own
        block), in the unit of the edges' information.  A pose's own block is
        exactly symmetric, block (a, b) is block (b, a) transposed bit for bit,
        rows and columns of held parameters are exactly 0.  The gauge is the
        caller's (hold one pose): np.linalg.LinAlgError when a pivot of the
        factor is not finite or L_rr^2 <= rank_tol H_rr.  device=True returns
        the device tensor without that host check (NaN blocks then;
        cov_status()).  Each distinct tile column max(a, b) // 10 costs one
        64-column solve and T 64x64 tiles of workspace (pg_cov_plan): ask for
        what is needed on a long trajectory.  Overwrites the LM workspace, not
        the poses or the LM state; iterate() rebuilds it."""
        out = []
        if poses is None and pairs is None:
            poses = np.arange(self.N)
        if poses is not None:
            c = np.asarray(poses)
            if c.ndim != 1 or c.dtype == np.bool_ or not np.issubdtype(c.dtype, np.integer) or len(c) == 0:
                raise ValueError("poses must be a non-empty list of integer pose indices")
            out.append(_cov_list(self.N, np.stack([c, c], 1), "poses"))
        if pairs is not None:
            out.append(_cov_list(self.N, pairs, "pairs"))
        pr = np.ascontiguousarray(np.concatenate(out), np.int32)
        rank_tol = _rank_tol(rank_tol)
        plan = pg_cov_plan(self.N, pr)
        dev = self.t["state"].device
        with torch.cuda.stream(self.stream if self.stream is not None else torch.cuda.current_stream()):
            ws = self._cov_ws(len(plan["cols"]))
            tp = torch.from_numpy(pr).to(dev)
            cov = torch.empty((len(pr), 6, 6), dtype=torch.float64, device=dev)
            _lib.call("slam_pg_covariance", ctypes.byref(self._s), ptr(tp), pr.ctypes.data, len(pr), rank_tol,
                      ptr(cov), ptr(ws), ws.numel(), ptr(self._cov_status), self._sp())
            if device:
                return cov
            host = cov.cpu().numpy()
        self._cov_raise(rank_tol)
        return host

    def gate(self, edges, meas, information=None, sqrt_information=None, rank_tol=1e-8, chi2=CHI2_6_99):
        """Is a proposed edge consistent with the graph?  For candidates k =
        (i, j) of `edges` [m, 2] with measurements `meas` [m, 6] (z = T_i^-1
        T_j, relative_pose) -- which need not be edges of the graph -- the raw
        residual e [m, 6] at the live poses, its first-order covariance under
        the graph P [m, 6, 6] (J_i S_ii J_i^T + J_i S_ij J_j^T + its transpose
        + J_j S_jj J_j^T over the blocks of covariance()), and the squared
        Mahalanobis distance d2 [m] = e^T (P + R)^-1 e with R the inverse of
        the candidate's information (`information` [m, 6, 6], factored as in
        the constructor, or `sqrt_information`; neither: R = 0).  accept =
        d2 <= chi2 (default: the 0.99 quantile of chi^2 with 6 degrees of
        freedom).  A candidate whose P + R fails rank_tol's rule (both poses
        held and R = 0) has d2 = NaN and is not accepted (gate_undetermined()).
        LinAlgError, cost and what is overwritten: as covariance()."""
        cand = _cov_list(self.N, edges, "edges", distinct=True)
        z = np.ascontiguousarray(np.asarray(meas, np.float64).reshape(-1, 6))
        if len(z) != len(cand):
            raise ValueError("meas must hold 6 values per candidate")
        if information is not None and sqrt_information is not None:
            raise ValueError("give information or sqrt_information, not both")
        A = None
        if information is not None:
            info = np.asarray(information, np.float64).reshape(len(cand), 6, 6)
            A = np.stack([np.linalg.cholesky(m).T for m in info])
        elif sqrt_information is not None:
            A = np.asarray(sqrt_information, np.float64).reshape(len(cand), 6, 6)
        if not np.all(np.isfinite(z)) or (A is not None and not np.all(np.isfinite(A))):
            raise ValueError("meas and the information must be finite")
        chi2 = float(chi2)
        if not chi2 > 0.0:
            raise ValueError(f"chi2 must be positive, not {chi2!r}")
        rank_tol = _rank_tol(rank_tol)
        plan = pg_cov_plan(self.N, cand, gate=True)
        dev = self.t["state"].device
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        m = len(cand)
        with torch.cuda.stream(self.stream if self.stream is not None else torch.cuda.current_stream()):
            ws = self._cov_ws(len(plan["cols"]))
            tc, tz, tA = T(cand), T(z), (T(A) if A is not None else None)
            d2 = torch.empty(m, dtype=torch.float64, device=dev)
            P = torch.empty((m, 6, 6), dtype=torch.float64, device=dev)
            e = torch.empty((m, 6), dtype=torch.float64, device=dev)
            _lib.call("slam_pg_gate", ctypes.byref(self._s), ptr(tc), cand.ctypes.data, ptr(tz), ptr(tA), m,
                      rank_tol, ptr(d2), ptr(P), ptr(e), ptr(ws), ws.numel(), ptr(self._cov_status), self._sp())
            d2, P, e = d2.cpu().numpy(), P.cpu().numpy(), e.cpu().numpy()
        self._cov_raise(rank_tol)
        return dict(d2=d2, P=P, e=e, accept=d2 <= chi2)

    def relative_covariance(self, pairs, rank_tol=1e-8):
        """First-order covariance [m, 6, 6] of relative_pose(x_i, x_j) for the
        (i, j) of `pairs`, i != j, under the graph: the gate's P with zero
        measurements and no information."""
        pr = _cov_list(self.N, pairs, "pairs", distinct=True)
        return self.gate(pr, np.zeros((len(pr), 6)), rank_tol=rank_tol)["P"]
