"""GPU Levenberg-Marquardt bundle adjustment (BAL model) — the device driver.

A reference-style BA problem (BundleAdjustment.py:331: params = [cams (C x 9),
points (P x 3)], cam_idxs, Q_idxs, qs) is planned by ba_plan (the index tables
the HIP kernels in csrc/ba*.hip consume; every planner name is re-exported
here); this module allocates the device buffers (torch tensors as HBM
containers, laid out by libslam355: _Layout), fills the slam_ba_problem
descriptor (_describe) and runs LM iterations with all state on the device.
Multi-GPU: each rank builds a BAProblem over ALL cameras and the observations
of its own points; `step_distributed` all-reduces the reduced camera system
(one RCCL all-reduce of ~(9C)^2 doubles) and two scalars per iteration.

Held parameters: `fixed` (BAProblem, BAWindowSet.build / stage) names camera
parameters that stay constant -- the gauge (the oldest keyframes held whole) or
a calibrated camera's f, k1, k2 (FIXED_INTRINSICS); see fixed_mask.  Every rank
of a sharded problem must pass the same mask.

Robust loss: `loss`, `f_scale` (BAProblem, BAWindowSet.build / stage) weigh
every observation by a robust kernel of its 2-vector reprojection error
(LOSSES, loss_args: scipy's names and rho).  Every rank of a
sharded problem must pass the same loss.

Covariance: `BAProblem.covariance` / `BABatch.covariance` (cov_pairs) return
marginal 9x9 covariance blocks of the camera parameters at the live
parameters, from the reduced camera system at zero damping, inverted on the
device.  The caller fixes the gauge with `fixed`.
`BAProblem.point_covariance` / `BABatch.point_covariance` (cov_points,
cov_cross) add the landmark blocks (3x3) and landmark-camera blocks (3x9) of
the same inverse, `BAProblem.reprojection_covariance` the 2x2 covariance of a
landmark's predicted pixel in a camera.
"""
from __future__ import annotations

import collections
import ctypes

import numpy as np
import torch

from . import _lib
from .device import ptr, require_gpu, stream_ptr

from ._lib import BAProblemStruct as _Prob
# the planners (pure host code) live in ba_plan; every name stays reachable here
from .ba_plan import (EPI_CAMS_MAX, GROUP_OBS, LDS_MAX_N, MF_CAMS, MF_CHUNK_OBS,  # noqa: F401
                      MF_CHUNK_PTS, TB, TILE_MODE, _INDEX_TABLES, _MFMA_TABLES, _flow_rs_order,
                      _pairs_by_point, _popcount, assembly_table, block_index, packed, plan,
                      plan_mfma, plan_mfma_native, point_groups, tile_rows, tiled_solve_flops,
                      tl_schedule, upper_blocks)

ST = dict(LAMBDA=0, NU=1, COST=2, COST_NEW=3, PRED=4, RHO=5, ACCEPTED=6, CUR=7, ITERS=8,
          NACCEPT=9, PRED_CAM=10, CHOL_FAIL=11, SOLVE_FAULT=16)
N_STATE = 20  # SLAM_BA_ST_SLOTS


def _check_indices(n_cams, n_pts, cam_idx, pt_idx, qs):
    cam_idx = np.asarray(cam_idx).astype(np.int64).ravel()
    pt_idx = np.asarray(pt_idx).astype(np.int64).ravel()
    qs = np.asarray(qs, np.float64).reshape(-1, 2)
    if not (len(cam_idx) == len(pt_idx) == len(qs)):
        raise ValueError("cam_idxs, Q_idxs and qs must have the same length")
    if len(cam_idx) and (cam_idx.min() < 0 or cam_idx.max() >= n_cams):
        raise ValueError("camera index out of range")
    if len(pt_idx) and (pt_idx.min() < 0 or pt_idx.max() >= n_pts):
        raise ValueError("point index out of range")
    return cam_idx, pt_idx, qs


# ----------------------------------------------------------------------------- held parameters
FIXED_INTRINSICS = np.array([0, 0, 0, 0, 0, 0, 1, 1, 1], np.uint8)  # hold f, k1, k2
FIXED_CAMERA = np.ones(9, np.uint8)  # hold a camera whole (a gauge anchor)


def fixed_mask(n_cams, fixed):
    """The mask words of slam_ba_problem.cam_fixed: uint32 [n_cams], bit i
    (0..8: w0 w1 w2 t0 t1 t2 f k1 k2) set = parameter i of that camera is held.
    `fixed`: None (all free), a bool / 0-1 array [n_cams, 9], or a [9] pattern
    applied to every camera.  A held parameter's column leaves the Jacobian:
    its LM step is exactly zero, everything else about the iteration stays."""
    n_cams = int(n_cams)
    if fixed is None:
        return np.zeros(n_cams, np.uint32)
    f = np.asarray(fixed)
    if f.dtype != np.bool_:
        if f.dtype == object or not (np.issubdtype(f.dtype, np.integer) or
                                     np.issubdtype(f.dtype, np.floating)):
            raise ValueError("fixed must be a bool or 0/1 array")
        if not np.all((f == 0) | (f == 1)):
            raise ValueError("fixed must hold only 0 and 1 (or bool)")
    if f.shape == (9,):
        f = np.broadcast_to(f, (n_cams, 9))
    elif f.shape != (n_cams, 9):
        raise ValueError(f"fixed must have shape (9,) or ({n_cams}, 9), not {f.shape}")
    bits = (f != 0).astype(np.uint32) << np.arange(9, dtype=np.uint32)
    return np.ascontiguousarray(bits.sum(1, dtype=np.uint32))


# ----------------------------------------------------------------------------- robust loss
LOSSES = {"linear": 0, "huber": 1, "soft_l1": 2, "cauchy": 3}  # slam_ba_problem.loss


def loss_args(loss, f_scale=1.0):
    """(code, scale) of slam_ba_problem.loss / loss_scale.  loss: None or a
    name of LOSSES (scipy least_squares' names and rho(z), z = |r|^2 /
    f_scale^2 of an observation's clamped 2-vector residual; the cost is
    0.5 f_scale^2 sum rho(z), the step the Gauss-Newton / IRLS one on
    sqrt(rho') r, sqrt(rho') J).  f_scale: the residual norm in pixels where
    the loss turns over, finite and > 0.  None and "linear" give code 0, the
    plain 0.5 |r|^2 and the code path of a problem built without the keyword."""
    if loss is None:
        loss = "linear"
    if not isinstance(loss, str) or loss not in LOSSES:
        raise ValueError(f"loss must be one of {sorted(LOSSES)} or None, not {loss!r}")
    try:
        scale = float(f_scale)
    except (TypeError, ValueError):
        raise ValueError(f"f_scale must be a number, not {f_scale!r}") from None
    if not (np.isfinite(scale) and scale > 0.0):
        raise ValueError(f"f_scale must be finite and > 0, not {f_scale!r}")
    return LOSSES[loss], scale


# ----------------------------------------------------------------------------- covariance
def _cov_ints(a, what, bounds):
    """`a` as a contiguous int32 index list: [m] in [0, bounds[0]) for one
    bound, [m, k] with column j in [0, bounds[j]) for k bounds.  ValueError on
    a non-integer dtype (an empty input of any dtype passes), another shape or
    an index out of range."""
    k = len(bounds)
    a = np.asarray(a)
    if a.size == 0:
        a = np.zeros((0,) if k == 1 else (0, k), np.int64)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what} must be integer indices")
    if a.ndim != (1 if k == 1 else 2) or (k > 1 and a.shape[1] != k):
        raise ValueError(f"{what} must have shape {'[m]' if k == 1 else f'[m, {k}]'}, not {list(a.shape)}")
    a = a.astype(np.int64)
    for j, n in enumerate(bounds):
        col = a if k == 1 else a[:, j]
        if col.size and (col.min() < 0 or col.max() >= n):
            raise ValueError(f"{what}: index out of range [0, {n})")
    return np.ascontiguousarray(a.astype(np.int32))


def cov_pairs(n_cams, cameras=None, pairs=None):
    """The int32 [m, 2] block list of slam_ba_covariance: (a, a) for every
    camera a of `cameras` (their marginal blocks), then the (a, b) of `pairs`
    (cross blocks Cov(a, b); a == b is allowed).  None, None: every camera's
    own block.  Raises ValueError on an index outside [0, n_cams), a
    non-integer or wrongly shaped input, or an empty list."""
    n_cams = int(n_cams)
    if n_cams < 1:
        raise ValueError("n_cams must be >= 1")
    if cameras is None and pairs is None:
        cameras = np.arange(n_cams)
    out = []
    if cameras is not None:
        c = _cov_ints(cameras, "cameras", (n_cams,))
        out.append(np.stack([c, c], 1))
    if pairs is not None:
        out.append(_cov_ints(pairs, "pairs", (n_cams, n_cams)))
    out = np.concatenate(out)
    if len(out) == 0:
        raise ValueError("no covariance block requested")
    return np.ascontiguousarray(out)


def cov_points(n_pts, points=None):
    """The int32 [m] point list of slam_ba_covariance_points: `points` in the
    caller's numbering (None: every point, 0 .. n_pts - 1; an empty list:
    none).  An index may repeat.  Raises ValueError on an index outside
    [0, n_pts), a non-integer or an input that is not 1-D."""
    n_pts = int(n_pts)
    if n_pts < 0:
        raise ValueError("n_pts must be >= 0")
    if points is None:
        return np.arange(n_pts, dtype=np.int32)
    return _cov_ints(points, "points", (n_pts,))


def cov_cross(n_pts, n_cams, cross):
    """The int32 [k, 2] (point, camera) list of slam_ba_covariance_points
    (None or an empty list: none); the camera need not observe the point.
    Raises ValueError on a point outside [0, n_pts), a camera outside
    [0, n_cams), a non-integer or a shape other than [k, 2]."""
    n_pts, n_cams = int(n_pts), int(n_cams)
    if n_pts < 0 or n_cams < 1:
        raise ValueError("n_pts must be >= 0 and n_cams >= 1")
    if cross is None:
        return np.zeros((0, 2), np.int32)
    return _cov_ints(cross, "cross (point, camera)", (n_pts, n_cams))


PointCovariance = collections.namedtuple("PointCovariance", "points cross cameras")


# ----------------------------------------------------------------------------- buffers
class _Layout:
    """The float64 buffers of one problem as libslam355 lays them out
    (slam_ba_f64_layout, csrc/ba_layout.hpp -- the one statement of it; host
    only): `names` in memory order, `off[k]` the start of buffer k in doubles
    from the problem's first, `shape[k]` its shape, `total` the aligned length
    of the whole.  `sizes` = (C, P, O, n_grps, n_cslots, n_bslots, n_blocks);
    chol_len: slam_ba_chol_len of a tiled solve (9C > 120), else 0."""

    names = ("cams0", "pts0", "cams1", "pts1", "init_c", "init_p", "obs_q", "camrec0", "camrec1",
             "cpart", "bpart", "sys", "chol", "delta_c", "red_part", "small", "state")  # SLAM_BA_F64_*
    uploaded = names[:7]  # filled from the host; the rest start as zeros
    _cols = dict(cams0=9, pts0=3, cams1=9, pts1=3, init_c=9, init_p=3, obs_q=2)  # rows of 2-D buffers
    __slots__ = ("sizes", "off", "shape", "total")

    def __init__(self, sizes, chol_len=0):
        n = len(self.names)
        out = (ctypes.c_longlong * (2 * n + 1))()
        a = ctypes.addressof(out)
        _lib.call("slam_ba_f64_layout", *sizes, int(chol_len), a, a + 8 * n, a + 16 * n)
        self.sizes = tuple(sizes)
        self.off = dict(zip(self.names, out[n:2 * n]))
        self.shape = {k: (ln // self._cols[k], self._cols[k]) if k in self._cols else (ln,)
                      for k, ln in zip(self.names, out[:n])}
        self.total = out[2 * n]


# where a BAWindowSet window lies in the set's two buffers: the sizes of its
# _Layout, its first double, its first int32, its plan's length and tables
_Place = collections.namedtuple("_Place", "sizes o64 o32 nb offs")


def _i32_layout(plan_len):
    """(int32 words of a window whose plan has plan_len words -- the tables,
    the one-element stand-ins of the lin_mode-0 tables from plan_len on, the
    ticket, all zeros, rounded up --, the ticket's offset, the end of the
    zeros): slam_ba_i32_layout."""
    out = (ctypes.c_longlong * 2)()
    a = ctypes.addressof(out)
    return int(_lib.lib.slam_ba_i32_layout(plan_len, a, a + 8)), out[0], out[1]


def _fill_uploaded(h64, base, lay, cams, pts, obs_q):
    """The uploaded buffers of a problem laid out from h64[base] on: the
    parameters three times (two LM copies and the initial one) and the
    observations in plan order (none: the zeros already there)."""
    for k in lay.uploaded:
        a = obs_q if k == "obs_q" else cams if lay.shape[k][1] == 9 else pts
        o = base + lay.off[k]
        h64[o:o + a.size] = a.ravel()


def _describe(lay, pl, f64, i32, ticket, tl_mode=0):
    """The slam_ba_problem of a planned problem: `lay` its _Layout, `pl` its
    plan (mode, n_sgrps), f64(k) / i32(k) the device address of float64
    buffer / index table k, `ticket` that of the completion counter.  The
    optional fields (tl_sched, asm_*, and the call options of
    _set_call_options) stay zero."""
    s = _Prob()
    s.n_cams, s.n_pts, s.n_obs, s.n_grps, s.n_cslots, s.n_bslots, s.n_blocks = lay.sizes
    s.lin_mode, s.n_sgrps, s.tl_mode = pl["mode"], pl["n_sgrps"], tl_mode
    s.cams[0], s.cams[1] = f64("cams0"), f64("cams1")
    s.pts[0], s.pts[1] = f64("pts0"), f64("pts1")
    s.camrec[0], s.camrec[1] = f64("camrec0"), f64("camrec1")
    for k in ("obs_q", "cpart", "bpart", "sys", "chol", "delta_c", "red_part", "small", "state"):
        setattr(s, k, f64(k))
    for k in _INDEX_TABLES + (_MFMA_TABLES if pl["mode"] == 1 else ()):
        setattr(s, k, i32(k))
    s.ticket = ticket
    return s


def _set_call_options(s, fdev, code, scale):
    """The fields of a descriptor that a call's keywords set: the held-parameter
    words (`fdev`: their device tensor, or None) and the robust loss."""
    if fdev is not None:
        s.cam_fixed = fdev.data_ptr()
    s.loss, s.loss_scale = code, scale


def _captured(owner, key, fn):
    """The HIP graph of fn()'s launches on `owner.stream`, captured on first
    use (on a fresh stream, as capture needs a non-default one, with
    owner.stream swapped for it) and kept in owner._graphs[key]."""
    graphs = owner.__dict__.setdefault("_graphs", {})
    if key not in graphs:
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        saved, owner.stream = owner.stream, s
        try:
            with torch.cuda.graph(g, stream=s):
                fn()
        finally:
            owner.stream = saved
        torch.cuda.current_stream().wait_stream(s)
        graphs[key] = g
    return graphs[key]


def _stream_of(owner):
    return torch.cuda.stream(owner.stream if owner.stream is not None else torch.cuda.current_stream())


class BAProblem:
    """Device-resident BA problem + LM state.  `cams` [C,9], `pts` [P,3] float64."""

    def __init__(self, cams, pts, cam_idx, pt_idx, qs, *, lam0=1e-4, stream=None,
                 block_list=None, lin_mode="auto", chunks_per_wg=None, tl_mode="flow",
                 fold_assembly=False, tile_mode=None, active_blocks=True, fixed=None,
                 loss=None, f_scale=1.0):
        """loss, f_scale: robust loss per observation (loss_args: None /
        "linear", "huber", "soft_l1", "cauchy"; f_scale in pixels); `prob.loss`
        is the name, `prob.f_scale` the scale.  COST / COST_NEW of state() are
        then 0.5 f_scale^2 sum rho(z); residuals() stays raw.
        fixed: camera parameters held constant (fixed_mask: None, a [9]
        pattern such as FIXED_INTRINSICS, or [C, 9]); `prob.fixed` is the
        uint32 [C] mask (None when nothing is held).  With None every result
        is the one a problem without the keyword gives.
        lin_mode: "mfma" (camera-union linearisation, k_lin_mfma: Schur
        contraction on the f64 matrix cores; points renumbered internally),
        "slot" (k_linearize, any observation structure) or "auto" (mfma when
        every point is seen by <= MF_CAMS cameras).  The tiled camera solve
        (9C > 120) follows the nested-dissection schedule of tl_schedule;
        tl_mode "flow" runs it as one dataflow launch (k_tl3_flow, on any
        stream and CU mask), "levels" one launch pair per elimination-tree level;
        tile_mode: the tiling of that solve (tile_rows; default TILE_MODE).
        active_blocks (packed systems): k_assemble only over the blocks with
        partial rows here (a landmark shard); those workgroups also write the
        zeros of the other blocks and of the cameras without rows (no
        separate launch).
        fold_assembly (lin_mode mfma): k_lin_mfma's last supergroup per camera
        block sums the block's partial rows into the system (no k_assemble
        launch).  Off by default: measured slower (the workgroup that finishes
        last assembles every block it touched, a serial tail; 16 C3 windows
        326 vs 225 us per iteration, C4 406 vs 324 us, tracking 19.0k vs 19.9k
        frames/s, profiles/r4/fold_ab/ at f26058c; landmark shards at W = 8 too: C4
        296 vs 155 us, C5 903 vs 387 us per iteration, profiles/r6/asm_fold/)."""
        if tl_mode not in ("flow", "levels"):
            raise ValueError(f"tl_mode must be 'flow' or 'levels', not {tl_mode!r}")
        dev = require_gpu()
        cams = np.ascontiguousarray(cams, np.float64).reshape(-1, 9)
        pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        C, P = len(cams), len(pts)
        cam_idx, pt_idx, qs = _check_indices(C, P, cam_idx, pt_idx, qs)
        self.fixed = None if fixed is None else fixed_mask(C, fixed)
        code, self.f_scale = loss_args(loss, f_scale)
        self.loss = "linear" if loss is None else loss
        pl = None
        if lin_mode in ("auto", "mfma"):
            pl = plan_mfma_native(C, P, cam_idx, pt_idx, block_list, chunks_per_wg)
            if pl is None and lin_mode == "mfma":
                raise ValueError(f"lin_mode 'mfma': a point is seen by more than {MF_CAMS} cameras")
        elif lin_mode != "slot":
            raise ValueError(f"lin_mode must be 'auto', 'mfma' or 'slot', not {lin_mode!r}")
        if pl is None:
            pl = plan(C, P, cam_idx, pt_idx, block_list)
            pl["mode"], pl["perm"] = 0, None
            pl["n_grps"], pl["n_sgrps"] = len(pl["grp_ptr"]) - 1, 0
        self.plan = pl
        self.lin_mode = "mfma" if pl["mode"] == 1 else "slot"
        self.perm = pl["perm"]  # device point k = caller's point perm[k] (None: identity)
        if self.perm is not None:
            pts = pts[self.perm]
        self.C, self.P, self.O = C, P, pl["n_obs"]
        self.stream = stream
        T = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.t = t = {}
        if "buf" in pl:  # native plan: every table in one buffer, one copy
            t["plan_buf"] = T(pl["buf"])
            for k in _INDEX_TABLES + _MFMA_TABLES:
                if k in pl["offs"]:
                    t[k] = t["plan_buf"][pl["offs"][k]:]  # (a zero-length table keeps its slot)
                else:
                    t[k] = T(pl[k].astype(np.int32))
        else:
            for k in _INDEX_TABLES + (_MFMA_TABLES if pl["mode"] == 1 else ()):
                arr = pl[k] if pl[k].size else np.zeros(1, np.int32)
                t[k] = T(arr.astype(np.int32))
        self.tl_levels = 9 * C > LDS_MAX_N
        chol_len = 0
        if self.tl_levels:  # schedule of the tiled solve (host copy; device copy below)
            self._sched_host = tl_schedule(C, pl["blocks"], tile_mode)
            chol_len = _lib.lib.slam_ba_chol_len(C, self._sched_host.ctypes.data)
        # every float64 buffer in ONE device allocation (256-byte aligned
        # segments): the parameters (two LM copies + the initial copy) and the
        # permuted observations in one upload, the workspaces in one fill
        lay = _Layout((C, P, self.O, pl["n_grps"], len(pl["cslot_cam"]), len(pl["bslot_blk"]),
                       len(pl["blocks"])), chol_len)
        self.sys_len = lay.shape["sys"][0]
        n_up = lay.off[lay.names[len(lay.uploaded)]]
        host = np.zeros(n_up, np.float64)
        _fill_uploaded(host, 0, lay, cams, pts, qs[pl["order"]])
        arena = torch.empty(lay.total, dtype=torch.float64, device=dev)
        arena[:n_up].copy_(torch.from_numpy(host))
        arena[n_up:].zero_()
        t["f64_arena"] = arena
        for k in lay.names:
            t[k] = arena[lay.off[k]:lay.off[k] + int(np.prod(lay.shape[k]))].view(lay.shape[k])
        if self.tl_levels:
            t["tl_sched"] = T(self._sched_host)
        t["ticket"] = torch.zeros(1, dtype=torch.int32, device=dev)
        if self.fixed is not None:
            t["cam_fixed"] = T(self.fixed.view(np.int32))
        if stream is not None:  # the uploads and fills above ran on the current stream
            stream.wait_stream(torch.cuda.current_stream(dev))
        addr = lambda k: t[k].data_ptr()  # noqa: E731
        s = _describe(lay, pl, addr, addr, addr("ticket"), 0 if tl_mode == "flow" else 1)
        if self.tl_levels:
            s.tl_sched = t["tl_sched"].data_ptr()
            s.tl_sched_host = self._sched_host.ctypes.data
        _set_call_options(s, t.get("cam_fixed"), code, self.f_scale)
        if pl["mode"] == 1 and fold_assembly:  # k_lin_mfma assembles sys itself
            t["asm_tab"] = T(assembly_table(C, pl))
            s.asm_tab = t["asm_tab"].data_ptr()
        elif self.tl_levels and active_blocks:
            # a landmark shard lists the global blocks but has partial rows for few
            # of them: k_assemble runs over the blocks with rows here (C5 rank 0
            # of 8: 3000 workgroups -> ~400), which also write the zeros of the
            # rest (table: the listed blocks, a flag per block, a flag per camera)
            blk = np.asarray(pl["blocks"]).reshape(-1, 2)
            bp = np.asarray(pl["blk_bslot_ptr"])
            cp = np.asarray(pl["cam_cslot_ptr"])
            rows = bp[1:] > bp[:-1]
            diag = blk[:, 0] == blk[:, 1]
            rows[diag] |= cp[blk[diag, 0] + 1] > cp[blk[diag, 0]]
            act = np.nonzero(rows)[0].astype(np.int32)
            if 0 < len(act) < len(blk):
                camrows = np.zeros(C, np.int32)
                camrows[blk[diag & rows, 0]] = 1
                t["asm_act"] = T(np.concatenate([act, rows.astype(np.int32), camrows]))
                s.asm_act, s.n_asm_act = t["asm_act"].data_ptr(), len(act)
        self._s = s
        self.reset(lam0)

        self._init = (t["init_c"], t["init_p"])

    def restore(self, lam0=1e-4):
        """Reload the initial parameters and reset the LM state (device copies)."""
        self.t["cams0"].copy_(self._init[0])
        self.t["pts0"].copy_(self._init[1])
        self.reset(lam0)

    # -- primitive phases -------------------------------------------------------
    def _sp(self):
        return stream_ptr(self.stream)

    def reset(self, lam0=1e-4):
        _lib.call("slam_ba_reset", ctypes.byref(self._s), float(lam0), self._sp())

    def build_system(self):
        _lib.call("slam_ba_build_system", ctypes.byref(self._s), self._sp())

    def solve_step(self):
        _lib.call("slam_ba_solve_step", ctypes.byref(self._s), self._sp())

    def decide(self):
        _lib.call("slam_ba_decide", ctypes.byref(self._s), self._sp())

    def iterate(self, n: int = 1):
        """n LM iterations, no host synchronisation (single rank)."""
        _lib.call("slam_ba_iterate", ctypes.byref(self._s), int(n), self._sp())

    def iterate_graphed(self, n: int = 1):
        """n LM iterations replayed from a captured HIP graph (one launch for
        the 13n kernels; captured on first use for each n)."""
        g = _captured(self, n, lambda: self.iterate(n))
        with _stream_of(self):
            g.replay()

    def _phase_graph(self, name, fn):
        """A captured HIP graph of one launch phase (captured on first use)."""
        return _captured(self, name, fn)

    def step_distributed(self, group=None, graphed=True, comm=None):
        """One LM iteration with RCCL all-reduce of the camera system (multi-rank).

        The kernels and the collectives are ordered on one stream: the body runs
        with self.stream current (torch.distributed orders its work against the
        current stream).  graphed: the linearisation (k_lin_mfma + k_assemble)
        and the solve (tiled factor + k_back_trial) are each one HIP-graph
        replay, so an iteration is 2 graph launches + k_decide + 2 collectives
        instead of ~8 kernel launches."""
        if comm is not None:  # slam355.dist.CapiComm: the whole iteration is one C call
            _lib.call("slam_ba_step_distributed", ctypes.byref(self._s), comm.handle, self._sp())
            return
        import torch.distributed as dist

        with _stream_of(self):
            if graphed:
                build = self._phase_graph("build", self.build_system)
                solve = self._phase_graph("solve", self.solve_step)
                build.replay()
                dist.all_reduce(self.t["sys"], group=group)
                solve.replay()
            else:
                self.build_system()
                dist.all_reduce(self.t["sys"], group=group)
                self.solve_step()
            dist.all_reduce(self.t["small"], group=group)
            self.decide()

    # -- host views ---------------------------------------------------------------
    def state(self) -> dict:
        """The LM state; raises SlamError when a dataflow camera solve ever
        timed out in one of its flag waits (SOLVE_FAULT, fail code 2).  The
        solve makes no residency assumption (a start ticket hands out columns,
        the last retirer forms x), so a timeout means a hang or a hand-off
        ordering bug in the kernel, not a launch that was not co-resident."""
        s = self.t["state"].cpu().numpy()
        st = {k: float(s[v]) for k, v in ST.items()}
        if st["SOLVE_FAULT"] != 0.0:
            raise _lib.SlamError(f"BA camera solve: a dataflow wait timed out (fail code 2) "
                                 f"{int(st['SOLVE_FAULT'])} time(s) -- a hang or hand-off ordering "
                                 "bug in k_tl3_flow; the affected LM steps were rejected")
        return st

    def params(self):
        """(cams [C,9], pts [P,3]) at the live parameters, points in the caller's order."""
        cur = int(self.t["state"][ST["CUR"]].item() != 0)
        cams = self.t[f"cams{cur}"].cpu().numpy().copy()
        pts = self.t[f"pts{cur}"].cpu().numpy()
        if self.perm is not None:
            out = np.empty_like(pts)
            out[self.perm] = pts
            pts = out
        return cams, pts.copy()

    def cost(self) -> float:
        return self.state()["COST"]

    def covariance(self, cameras=None, pairs=None, scale="unit", rank_tol=1e-8, device=False):
        """Marginal covariance blocks of the camera parameters at the live
        parameters: [m, 9, 9] float64 in the order of cov_pairs(C, cameras,
        pairs) -- Cov(a, a) per camera of `cameras`, then Cov(a, b) per pair
        (None, None: every camera's own block).  They are blocks of S0^-1, S0
        the Schur-reduced camera system with zero damping of the clamped,
        masked, robust-weighted Jacobian of the LM steps; rows
        and columns of held parameters are exactly 0.
        scale: "unit" (unit-variance pixel noise), "residual" (times
        2 COST / (2 O - n_free), n_free = free camera parameters + 3 P), or a
        positive float.  The gauge must be fixed by the caller (`fixed`: two
        cameras held whole suffice): np.linalg.LinAlgError when S0 is not
        numerically positive definite, i.e. a Cholesky pivot L_kk^2 <=
        rank_tol S0_kk or not finite.  device=True returns the device tensor
        without that host check (NaN blocks then; cov_status() reads the
        status of the last call).  A point whose 3x3 block is singular
        without damping counts with a zero inverse, as in the LM steps.
        The landmark blocks of the same inverse: point_covariance().  A
        landmark shard's system is not summed over ranks here.
        Overwrites `sys`: a build_system() made before the call must be
        repeated before solve_step() (iterate* rebuilds anyway); the LM state
        and the parameters are untouched.  The workspace (two dense tiled
        matrices) is allocated on first use and kept."""
        pr = cov_pairs(self.C, cameras, pairs)
        fac, rank_tol = self._cov_args(scale, rank_tol)
        s = self._s  # (a BAWindowSet problem: raises once its buffers were reused)
        dev = self.t["state"].device
        with torch.cuda.stream(self.stream if self.stream is not None else torch.cuda.current_stream()):
            self._cov_buffers(dev)
            tp = torch.from_numpy(pr).to(dev)
            out = torch.empty((len(pr), 9, 9), dtype=torch.float64, device=dev)
            _lib.call("slam_ba_covariance", ctypes.byref(s), ptr(tp), len(pr), rank_tol, ptr(out),
                      ptr(self._cov_ws), self._cov_ws.numel(), ptr(self._cov_status), self._sp())
            if scale == "residual":
                fac = self._cov_residual_factor()
            if fac is not None:
                out *= fac
            if device:
                return out
            host = out.cpu().numpy()
        self._cov_raise(rank_tol)
        return host

    @staticmethod
    def _cov_args(scale, rank_tol):
        """(factor or None for "unit" / "residual", rank_tol), checked."""
        if isinstance(scale, str):
            if scale not in ("unit", "residual"):
                raise ValueError(f"scale must be 'unit', 'residual' or a positive float, not {scale!r}")
            fac = None
        else:
            fac = float(scale)
            if not (np.isfinite(fac) and fac > 0.0):
                raise ValueError(f"scale must be 'unit', 'residual' or a positive float, not {scale!r}")
        rank_tol = float(rank_tol)
        if not (np.isfinite(rank_tol) and 0.0 <= rank_tol < 1.0):
            raise ValueError(f"rank_tol must be finite and in [0, 1), not {rank_tol!r}")
        return fac, rank_tol

    def _cov_buffers(self, dev):
        if getattr(self, "_cov_ws", None) is None:
            n = int(_lib.lib.slam_ba_cov_workspace_len(self.C))
            self._cov_ws = torch.empty(n, dtype=torch.float64, device=dev)
            self._cov_status = torch.zeros(2, dtype=torch.int32, device=dev)

    def _cov_residual_factor(self):
        n_free = 9 * self.C + 3 * self.P
        if self.fixed is not None:
            n_free -= sum(_popcount(int(w) & 0x1FF) for w in self.fixed)
        dof = 2 * self.O - n_free
        if dof <= 0:
            raise ValueError(f"scale 'residual': 2 O - n_free = {dof} degrees of freedom")
        return 2.0 * self.state()["COST"] / dof

    def _cov_raise(self, rank_tol):
        if self.cov_status() != 0:
            raise np.linalg.LinAlgError(
                "BA covariance: the reduced camera system is not positive definite at "
                f"rank_tol {rank_tol:g} (fix the gauge: hold two cameras whole)")

    def cov_status(self) -> int:
        """Status of the last covariance() / point_covariance() call: 0 ok, 1 not positive definite."""
        return int(self._cov_status[0].item())

    def cov_undetermined(self) -> int:
        """Rows of the last point_covariance() call that are NaN because their
        point is undetermined."""
        return int(self._cov_status[1].item())

    def point_covariance(self, points=None, cross=None, cameras=None, pairs=None, scale="unit",
                         rank_tol=1e-8, device=False):
        """Landmark, landmark-camera and camera blocks of the covariance at the
        live parameters, from one build and one factorisation: the named tuple
        PointCovariance(points [m, 3, 3], cross [k, 3, 9], cameras [n, 9, 9]),
        float64.  They are blocks of (J~^T J~)^-1 over the free parameters, J~
        the clamped, masked, robust-weighted Jacobian of the LM steps
        (DESIGN.md 4c).
        points: point indices in the caller's numbering (cov_points; None:
        every point, []: none) -> Cov(point, point), exactly symmetric.
        cross: (point, camera) pairs (cov_cross; None: none) -> Cov(point,
        camera); the camera need not observe the point; columns of held
        parameters are exactly 0.
        cameras, pairs: as covariance(), except that None, None asks for no
        camera block.  An index may repeat in any list.
        scale, rank_tol, device and the LinAlgError on a reduced camera system
        that is not positive definite: as covariance().  A point is
        undetermined when a pivot of the 3x3 Cholesky of its V = sum Jp^T Jp
        is not finite or <= rank_tol V_kk (no or one observation, rays nearly
        parallel): its rows are NaN, cov_undetermined() counts them, nothing
        is raised.  (The camera blocks still see such a point as the LM steps
        do: leave one-observation points out of a problem whose camera
        covariance matters.)  Overwrites `sys` like covariance()."""
        inv = None
        if self.perm is not None:  # device point k = caller's point perm[k]
            inv = np.empty(self.P, np.int32)
            inv[self.perm] = np.arange(self.P, dtype=np.int32)
        every = points is None and inv is None
        pts = cov_points(self.P, points)
        cr = cov_cross(self.P, self.C, cross)
        if inv is not None:
            pts = inv[pts]
            cr = np.stack([inv[cr[:, 0]], cr[:, 1]], 1)
        n_cam_req = sum(0 if x is None else np.size(x) for x in (cameras, pairs))
        pr = cov_pairs(self.C, cameras, pairs) if n_cam_req else np.zeros((0, 2), np.int32)
        fac, rank_tol = self._cov_args(scale, rank_tol)
        s = self._s  # (a BAWindowSet problem: raises once its buffers were reused)
        dev = self.t["state"].device
        with torch.cuda.stream(self.stream if self.stream is not None else torch.cuda.current_stream()):
            self._cov_buffers(dev)
            lists = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (pr, pts, cr)]
            outs = [torch.empty((len(a),) + shp, dtype=torch.float64, device=dev)
                    for a, shp in ((pr, (9, 9)), (pts, (3, 3)), (cr, (3, 9)))]
            if len(pr) + len(pts) + len(cr):
                lp = [ptr(t) if t.numel() else None for t in lists]
                if every:
                    lp[1] = None  # the all-points form: no list
                _lib.call("slam_ba_covariance_points", ctypes.byref(s), lp[0], len(pr), ptr(outs[0]),
                          lp[1], len(pts), ptr(outs[1]), lp[2], len(cr), ptr(outs[2]), rank_tol,
                          ptr(self._cov_ws), self._cov_ws.numel(), ptr(self._cov_status), self._sp())
            else:
                self._cov_status.zero_()
            if scale == "residual":
                fac = self._cov_residual_factor()
            if fac is not None:
                for o in outs:
                    o *= fac
            if not device:
                outs = [o.cpu().numpy() for o in outs]
        if not device:
            self._cov_raise(rank_tol)
        return PointCovariance(outs[1], outs[2], outs[0])

    def reprojection_covariance(self, points, cameras):
        """[m, 2, 2]: the covariance of the predicted pixel of point points[i]
        in camera cameras[i] at the live parameters, A [S_cc S_cp; S_pc S_pp] A^T
        with A = (A_c | A_p) the raw 2 x 12 Jacobian of the projection (no
        clamp, no mask, no robust weight) and the blocks of one
        point_covariance() call (unit scale).  The camera need not observe the
        point.  Exactly symmetric; NaN for an undetermined point."""
        pts = cov_points(self.P, points)
        cam = _cov_ints(cameras, "cameras", (self.C,))
        if len(pts) != len(cam):
            raise ValueError("points and cameras must have the same length")
        if len(pts) == 0:
            return np.zeros((0, 2, 2))
        cov = self.point_covariance(points=pts, cross=np.stack([pts, cam], 1), cameras=cam)
        lc, lp = self.params()
        # q = the projection itself: the residual is 0 and the clamp inactive
        q = residuals(lc, lp, cam, pts, np.zeros((len(pts), 2)))
        r, A = residuals(lc, lp, cam, pts, q, jacobian=True)
        if np.any(r != 0.0):  # the first pass was clamped (a pixel beyond 5000): one more step
            q = q + r
            r, A = residuals(lc, lp, cam, pts, q, jacobian=True)
        S = np.empty((len(pts), 12, 12))
        S[:, :9, :9], S[:, 9:, 9:] = cov.cameras, cov.points
        S[:, 9:, :9] = cov.cross
        S[:, :9, 9:] = cov.cross.transpose(0, 2, 1)
        R = A @ S @ A.transpose(0, 2, 1)
        return 0.5 * (R + R.transpose(0, 2, 1))

    def solve(self, max_iters=100, ftol=1e-10, check_every=5):
        """Iterate until a batch of `check_every` iterations that accepted at
        least one step lowered the cost by less than ftol (relative), until
        lambda saturates (no step can be accepted any more), or max_iters.
        A batch whose steps were all rejected leaves the cost unchanged and
        says nothing about convergence, so it never stops the solve.
        Returns the final state dict."""
        done = 0
        st = self.state()
        while done < max_iters:
            k = min(check_every, max_iters - done)
            c0, n0 = st["COST"], st["NACCEPT"]
            self.iterate(k)
            done += k
            st = self.state()
            if st["LAMBDA"] >= 1e30:
                break
            if st["NACCEPT"] > n0 and abs(c0 - st["COST"]) <= ftol * max(st["COST"], 1e-300):
                break
        return st


class BABatch:
    """Independent BA problems (e.g. the local-BA windows of one tracking
    batch) advanced together: each LM iteration of all of them is one set of
    launches (slam_ba_iterate_batch: one problem per grid row, up to
    SLAM_BA_MAX_BATCH per launch), so B windows cost about one window's
    latency instead of B.  Every problem keeps its own device buffers and LM
    state; its iterates equal the ones BAProblem.iterate gives it alone."""

    MAX_BATCH = 16  # SLAM_BA_MAX_BATCH

    def __init__(self, problems, stream=None):
        self.problems = list(problems)
        if not self.problems:
            raise ValueError("BABatch needs at least one problem")
        if len(self.problems) > 1 and any(packed(p.C) for p in self.problems):
            raise ValueError(f"batched problems must have 9C <= {LDS_MAX_N} (one-workgroup solver)")
        self.stream = stream
        arr = (_Prob * len(self.problems))()
        for i, p in enumerate(self.problems):
            ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(p._s), ctypes.sizeof(_Prob))
        self._arr = arr
        # BAWindowSet problems: checked before every launch (their buffers are
        # reused two stage()/build() calls later)
        self._win = [p for p in self.problems if hasattr(p, "_live")]

    def _sp(self):
        return stream_ptr(self.stream)

    def reset(self, lam0=1e-4):
        _lib.call("slam_ba_reset_batch", self._arr, len(self.problems), float(lam0), self._sp())

    def restore(self, lam0=1e-4):
        """Reload every problem's initial parameters, reset every LM state."""
        with _stream_of(self):
            # one multi-tensor copy launch for all windows: captured in a graph,
            # 2 copies per window were 2 memcpy nodes each, dispatched ~55 us
            # apart on a busy device (1 ms per launch set of 8 windows)
            torch._foreach_copy_([t for p in self.problems for t in (p.t["cams0"], p.t["pts0"])],
                                 [t for p in self.problems for t in p._init])
        self.reset(lam0)

    def iterate(self, n: int = 1):
        for p in self._win:
            p._live()
        _lib.call("slam_ba_iterate_batch", self._arr, len(self.problems), int(n), self._sp())

    def iterate_graphed(self, n: int = 1, with_restore=False):
        """n LM iterations of every problem (optionally preceded by restore())
        replayed from one captured HIP graph."""
        for p in self._win:
            p._live()
        def body():
            if with_restore:
                self.restore()
            self.iterate(n)

        g = _captured(self, (n, with_restore), body)
        with _stream_of(self):
            g.replay()

    def states(self):
        return [p.state() for p in self.problems]

    def covariance(self, cameras=None, pairs=None, scale="unit", rank_tol=1e-8, device=False):
        """BAProblem.covariance of every problem, one after the other (a host
        loop: not a per-iteration path); a list, one entry per problem."""
        return [p.covariance(cameras, pairs, scale, rank_tol, device) for p in self.problems]

    def point_covariance(self, points=None, cross=None, cameras=None, pairs=None, scale="unit",
                         rank_tol=1e-8, device=False):
        """BAProblem.point_covariance of every problem, one after the other; a
        list of PointCovariance, one per problem (the same request for each)."""
        return [p.point_covariance(points, cross, cameras, pairs, scale, rank_tol, device)
                for p in self.problems]


# ----------------------------------------------------------------------------- kernels
def residuals(cams, pts, cam_idx, pt_idx, qs, *, jacobian=False):
    """objective()-order residuals [O,2] (and Jacobians [O,2,12]) on the GPU."""
    dev = require_gpu()
    cams = np.ascontiguousarray(cams, np.float64).reshape(-1, 9)
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    cam_idx, pt_idx, qs = _check_indices(len(cams), len(pts), cam_idx, pt_idx, qs)
    O = len(cam_idx)
    if O == 0:
        return (np.zeros((0, 2)), np.zeros((0, 2, 12))) if jacobian else np.zeros((0, 2))
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    tc, tp = T(cams), T(pts)
    ti, tj, tq = T(cam_idx.astype(np.int32)), T(pt_idx.astype(np.int32)), T(qs)
    r = torch.empty((O, 2), dtype=torch.float64, device=dev)
    if jacobian:
        J = torch.empty((O, 2, 12), dtype=torch.float64, device=dev)
        _lib.call("slam_ba_jacobian", ptr(tc), ptr(tp), ptr(ti), ptr(tj), ptr(tq), O, ptr(r),
                  ptr(J), stream_ptr())
        return r.cpu().numpy(), J.cpu().numpy()
    _lib.call("slam_ba_residual", ptr(tc), ptr(tp), ptr(ti), ptr(tj), ptr(tq), O, ptr(r),
              stream_ptr())
    return r.cpu().numpy()


class _WindowProblem(BAProblem):
    """A BAProblem whose buffers are views into a BAWindowSet's device memory
    (built by BAWindowSet.build / stage, not by __init__).  The kernels see raw
    pointers set at build time; the torch views (`t`, `_init`) that the
    BAProblem methods read are made on first use only.

    Lifetime: the set double-buffers its device memory, so the problems of one
    call stay valid through the next call; the call after that reuses their
    buffers, and from then on every use of them (launches, `state()`,
    `params()`, a new BABatch over them) raises RuntimeError instead of
    silently reading another batch's data."""

    def __init__(self):  # noqa: D107 (constructed by BAWindowSet only)
        pass

    def _live(self):
        if self._ws.gen[self._slot] != self._gen:
            raise RuntimeError("BAWindowSet problem used after its device buffers were reused "
                               "(problems stay valid for one further stage()/build() call)")

    @property
    def _s(self):
        self._live()
        return self._s_raw

    @property
    def t(self):
        self._live()
        if self._t is None:
            pc = self._where
            if not isinstance(pc, _Place):  # staged by BAWindowSet.stage: read from its meta row
                pc = self._where = BAWindowSet._placed(pc)
            lay = self._lay = self._lay or _Layout(pc.sizes)
            d64, d32 = self._d64, self._d32
            t = {}
            for k in lay.names:
                o, shp = pc.o64 + lay.off[k], lay.shape[k]
                t[k] = d64[o:o + int(np.prod(shp))].view(shp)
            pb = d32[pc.o32:pc.o32 + pc.nb]
            t["plan_buf"] = pb
            stand, ticket = pc.o32 + pc.nb, pc.o32 + _i32_layout(pc.nb)[1]
            for k in _INDEX_TABLES + _MFMA_TABLES + ("perm",):
                t[k] = pb[pc.offs[k]:] if k in pc.offs else d32[stand:stand + 1]
            t["ticket"] = d32[ticket:ticket + 1]
            self._t = t
        return self._t

    @property
    def _init(self):
        return (self.t["init_c"], self.t["init_p"])

    @property
    def perm(self):
        if self._perm is None:
            self._perm = self.t["perm"][:self.P].cpu().numpy().astype(np.int64)
        return self._perm

    @perm.setter
    def perm(self, v):
        self._perm = v


class BAWindowSet:
    """Many small BA problems built together for one launch set -- the local-BA
    windows formed from tracked frames (bench.py's tracked leg): each window
    planned by the native planner, every window's tables and float64 data
    (parameters, observations, zeroed workspaces: BAProblem's layout) staged in
    ONE pinned host buffer per type and uploaded by ONE asynchronous copy each,
    on the BA stream, into device buffers kept across calls; the returned
    problems have BAProblem's interface (state(), params(), BABatch).  Windows
    that need the slot linearisation (a point seen by more than MF_CAMS
    cameras) or the tiled solve (9C > 120) are built as ordinary BAProblems.

    Two sets of buffers alternate call by call -- pinned host staging and
    device memory alike -- so a call's problems stay valid through the next
    call (the bench's lag-2 pipeline launches step k's set while step k+1's
    is staged).  Set s is reused two calls later: its upload is ordered on
    `stream` after the launches of the problems it held (same stream), its
    host staging only after its previous upload has run (an event), and its
    generation is bumped, so the old problems then raise on any use
    (_WindowProblem._live) rather than read the new batch's data."""

    def __init__(self):
        self.dev = require_gpu()
        self.d = [[None, None], [None, None]]  # (f64, i32) device buffers per set
        self.h = [None, None]  # (f64, i32, event) host staging per set
        self.gen = [0, 0]  # calls that have filled each set
        self.k = 0
        self._fx = None  # (mask words, their device copy) of the last call with held parameters

    def _claim(self):
        """The set this call fills: its generation bumped (the problems of its
        previous fill are dead from here on)."""
        slot = self.k & 1
        self.gen[slot] += 1
        return slot

    def _claim_buffers(self, slot, need64, need32, stream):
        """(staging, device buffers) of set `slot` once its previous upload has
        run (the event), the pinned staging regrown by 3/2 when it has no room
        for need64 doubles / need32 int32, the device buffers kept at least as
        large as the staging.  Staging is None before the set's first fill
        when nothing is asked for."""
        hs, d = self.h[slot], self.d[slot]
        if hs is not None:
            hs[2].synchronize()
        have = (0, 0) if hs is None else (hs[0].numel(), hs[1].numel())
        if have[0] < need64 or have[1] < need32:
            hs = [torch.zeros(max(need64, 1) * 3 // 2, dtype=torch.float64, pin_memory=True),
                  torch.zeros(max(need32, 1) * 3 // 2, dtype=torch.int32, pin_memory=True),
                  torch.cuda.Event()]
            self.h[slot] = hs
        if hs is not None:
            with torch.cuda.stream(stream):
                for i, dt in enumerate((torch.float64, torch.int32)):
                    if d[i] is None or d[i].numel() < hs[i].numel():
                        d[i] = torch.empty(hs[i].numel(), dtype=dt, device=self.dev)
        return hs, d

    def _upload(self, slot, n64, n32, stream):
        """Set `slot`'s staged doubles and int32 to its device buffers, one
        asynchronous copy each on `stream`, the event after them; the next call
        fills the other set."""
        hs, d = self.h[slot], self.d[slot]
        self.k += 1
        with torch.cuda.stream(stream):
            if n64:
                d[0][:n64].copy_(hs[0][:n64], non_blocking=True)
            if n32:
                d[1][:n32].copy_(hs[1][:n32], non_blocking=True)
            hs[2].record(stream)

    def _adopt(self, slot, where, s, sizes, sys_len, stream, opts, lay=None, plan=None):
        """The _WindowProblem of a window of set `slot`: `where` its _Place (or
        the meta row _placed reads it from, on first use), `s` its descriptor,
        sizes = (C, P, O), opts = (mask words, their device copy, loss name,
        code, scale) of the call."""
        bp = _WindowProblem()
        bp._ws, bp._slot, bp._gen = self, slot, self.gen[slot]
        bp._d64, bp._d32 = self.d[slot]
        bp._where, bp._lay, bp._t = where, lay, None
        bp.plan, bp.lin_mode = plan, "mfma"
        bp.perm = None if plan is None else plan["perm"]  # (None: read back from the tables)
        bp.C, bp.P, bp.O = sizes
        bp.stream, bp.sys_len, bp.tl_levels = stream, sys_len, False
        fwords, bp._fixed_t, bp.loss, code, bp.f_scale = opts
        bp.fixed = None if fwords is None else fwords[:bp.C]
        _set_call_options(s, bp._fixed_t, code, bp.f_scale)
        bp._s_raw = s
        return bp

    @staticmethod
    def _reset_built(out, lam0, stream):
        """The LM states of the set's own problems in `out`, reset together in
        launch-sized groups (after the upload: same stream)."""
        built = [p for p in out if isinstance(p, _WindowProblem)]
        for i in range(0, len(built), BABatch.MAX_BATCH):
            BABatch(built[i:i + BABatch.MAX_BATCH], stream=stream).reset(lam0)

    def _fixed_dev(self, sizes, fixed, stream):
        """The device mask words of a call whose windows have `sizes` cameras:
        one small buffer owned by the set, shared by the call's windows (a [9]
        pattern: a word per camera of the largest window; [n, 9]: every window
        has n cameras).  Kept while the mask stays the same and never
        rewritten -- a new mask gets a new buffer, which the problems that
        point at it keep alive -- so it needs no double buffering."""
        if fixed is None or not sizes:
            return None, None
        f = np.asarray(fixed)
        if f.ndim == 2 and any(c != f.shape[0] for c in sizes):
            raise ValueError(f"fixed [{f.shape[0]}, 9] needs windows of {f.shape[0]} cameras")
        words = fixed_mask(max(sizes), f)
        if self._fx is None or not np.array_equal(self._fx[0], words):
            with torch.cuda.stream(stream):
                self._fx = (words, torch.from_numpy(words.view(np.int32)).to(self.dev))
        return self._fx

    META = 12 + len(_Layout.names) + len(_lib.PLAN_TABLES)  # SLAM_STAGE_META

    @staticmethod
    def _placed(m):
        """The _Place of a window staged by slam_ba_stage_windows, from its
        meta row m (staged, C, P, O, n_grps, n_sgrps, n_cslots, n_bslots,
        n_blocks, int32 offset, plan length, sys length, the float64 offsets
        -- the window's first double leads them --, the plan table offsets)."""
        base = 12 + len(_Layout.names)
        offs = {k: int(m[base + i]) for i, k in enumerate(_lib.PLAN_TABLES)}
        sizes = tuple(int(m[i]) for i in (1, 2, 3, 4, 6, 7, 8))
        return _Place(sizes, int(m[12]), int(m[9]), int(m[10]), offs)

    def stage(self, rows, cnt, maps, M, cams, u_off, v_off, stream, lam0=1e-4, fixed=None,
              loss=None, f_scale=1.0):
        """The tracked windows of one batch, staged by ONE native call
        (slam_ba_stage_windows: every window's observations from the mapper's
        rows, its plan, its float64 data and tables into the pinned staging
        buffers, its descriptor with the device addresses) and uploaded by one
        copy per type.  rows [B, cap, 4] (frame, map point, u, v), cnt [B],
        maps [W, map_cap, 3], M [W], cams [B, 9] with B = W n; window w = pairs
        w n .. w n + n - 1.  Windows the camera-union plan cannot take are
        built as ordinary BAProblems (from the same host arrays).  Returns the
        problems in window order (BAProblem interface).  fixed: held camera
        parameters, one [9] or [n, 9] pattern for every window of the call
        (fixed_mask); its device words are written into the descriptors after
        the native call, whose staged layout does not change.  loss, f_scale:
        the robust loss of every window of the call (loss_args), written into
        the descriptors in the same place."""
        code, scale = loss_args(loss, f_scale)
        rows = np.ascontiguousarray(rows, np.float64)
        cnt = np.ascontiguousarray(cnt, np.int32)
        maps = np.ascontiguousarray(maps, np.float64)
        M = np.ascontiguousarray(M, np.int32)
        cams = np.ascontiguousarray(cams, np.float64).reshape(-1, 9)
        B, cap = rows.shape[0], rows.shape[1]
        W, map_cap = maps.shape[0], maps.shape[1]
        if W == 0 or B % W or len(cams) != B or len(cnt) != B or len(M) != W:
            raise ValueError("stage: rows / cnt / cams must cover W windows of B / W pairs each")
        n = B // W
        opts = (*self._fixed_dev([n], fixed, stream), "linear" if loss is None else loss, code, scale)
        meta = np.zeros((W, self.META), np.int64)
        need = np.zeros(2, np.int64)
        probs = (_Prob * W)()
        args = (W, n, cap, rows.ctypes.data, cnt.ctypes.data, maps.ctypes.data, map_cap,
                M.ctypes.data, cams.ctypes.data, float(u_off), float(v_off))
        slot = self._claim()
        hs, d = self._claim_buffers(slot, 0, 0, stream)  # as they are; none before the first fill
        for attempt in range(2):
            # fill what is there (no buffers: sizes only); when it has no room, grow and fill again
            bufs = (None, 0, None, 0, None, None, None) if hs is None else \
                (hs[0].data_ptr(), hs[0].numel(), hs[1].data_ptr(), hs[1].numel(), d[0].data_ptr(),
                 d[1].data_ptr(), ctypes.addressof(probs))
            _lib.call("slam_ba_stage_windows", *args, *bufs, meta.ctypes.data, need.ctypes.data)
            n64, n32 = int(need[0]), int(need[1])
            if hs is not None and n64 <= hs[0].numel() and n32 <= hs[1].numel():
                break
            hs, d = self._claim_buffers(slot, max(n64, 1), max(n32, 1), stream)
        else:
            raise RuntimeError("stage: staging buffers could not be sized")
        self._upload(slot, n64, n32, stream)
        out = []
        for w in range(W):
            m = meta[w]
            if not m[0]:  # not plannable here: an ordinary problem from the same rows
                om = np.concatenate([rows[b, :max(min(int(cnt[b]), cap), 0)] for b in range(w * n, w * n + n)])
                qs = np.stack([om[:, 2] - u_off, om[:, 3] - v_off], 1)
                out.append(BAProblem(cams[w * n:w * n + n].copy(), maps[w, :int(M[w])].copy(),
                                     om[:, 0].astype(np.int64), om[:, 1].astype(np.int64), qs,
                                     lam0=lam0, stream=stream, fixed=fixed, loss=loss, f_scale=f_scale))
                continue
            out.append(self._adopt(slot, m, probs[w], (int(m[1]), int(m[2]), int(m[3])), int(m[11]),
                                   stream, opts))
        self._reset_built(out, lam0, stream)
        return out

    def build(self, problems, stream, lam0=1e-4, fixed=None, loss=None, f_scale=1.0):
        """The windows `problems` [(cams, pts, cam_idx, pt_idx, qs), ...] built
        together (see the class); fixed: held camera parameters, one [9] or
        [n, 9] pattern shared by every window of the call (fixed_mask); loss,
        f_scale: the robust loss of every window of the call (loss_args)."""
        problems = list(problems)
        code, scale = loss_args(loss, f_scale)
        opts = (*self._fixed_dev([len(np.reshape(pr[0], (-1, 9))) for pr in problems], fixed, stream),
                "linear" if loss is None else loss, code, scale)
        specs, extra = [], []
        n64 = n32 = 0
        for w, (cams, pts, ci, pi, qs) in enumerate(problems):
            cams = np.ascontiguousarray(cams, np.float64).reshape(-1, 9)
            pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
            C, P = len(cams), len(pts)
            ci, pi, qs = _check_indices(C, P, ci, pi, qs)
            pl = plan_mfma_native(C, P, ci, pi) if 9 * C <= LDS_MAX_N else None
            if pl is None:
                extra.append(BAProblem(cams, pts, ci, pi, qs, lam0=lam0, stream=stream, fixed=fixed,
                                       loss=loss, f_scale=f_scale))
                continue
            if pl["perm"] is not None:
                pts = pts[pl["perm"]]
            lay = _Layout((C, P, pl["n_obs"], pl["n_grps"], len(pl["cslot_cam"]), len(pl["bslot_blk"]),
                           len(pl["blocks"])))
            nb = len(pl["buf"])
            w32, ticket, end = _i32_layout(nb)
            specs.append((w, cams, pts, qs[pl["order"]], pl, lay, ticket, end,
                          _Place(lay.sizes, n64, n32, nb, pl["offs"])))
            n64 += lay.total
            n32 += w32
        # staging (pinned, alternating sets) and device buffers (grown as needed)
        slot = self._claim()
        hs, d = self._claim_buffers(slot, max(n64, 1), max(n32, 1), stream)
        h64, h32 = hs[0].numpy(), hs[1].numpy()
        h64[:n64] = 0.0
        for w, cams, pts, obs_q, pl, lay, ticket, end, pc in specs:
            _fill_uploaded(h64, pc.o64, lay, cams, pts, obs_q)
            h32[pc.o32:pc.o32 + pc.nb] = pl["buf"]
            h32[pc.o32 + pc.nb:pc.o32 + end] = 0
        self._upload(slot, n64, n32, stream)
        out = [None] * len(problems)
        b64, b32 = d[0].data_ptr(), d[1].data_ptr()
        for w, cams, pts, obs_q, pl, lay, ticket, end, pc in specs:
            # raw pointers from the offsets (no torch view per buffer: ~30 per
            # window were most of the host build); the views are made on demand
            s = _describe(lay, pl, lambda k: b64 + 8 * (pc.o64 + lay.off[k]),
                          lambda k: b32 + 4 * (pc.o32 + pc.offs.get(k, pc.nb)),
                          b32 + 4 * (pc.o32 + ticket))
            out[w] = self._adopt(slot, pc, s, lay.sizes[:3], lay.shape["sys"][0], stream, opts, lay, pl)
        it = iter(extra)
        out = [p if p is not None else next(it) for p in out]
        self._reset_built(out, lam0, stream)
        return out

