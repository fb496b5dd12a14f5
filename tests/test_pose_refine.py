"""Robust pose refinement from guided matches: slam_pose_refine,
geometry.refine_pose and LandmarkMap.localize against tests/pose_refine_ref.py
(a NumPy restatement of the header's definition).

Bars: status, inlier count and mask equal (the scenes keep every |r|^2 a
relative 1e-6 away from gate^2 at every classification the reference makes, so
a mask difference is no rounding coin toss); the pose at the project's PnP bar
(rotation entries 1e-8, translation 1e-8 (1 + max|t|)); the cost to 1e-8
relative (plus the rounding floor of _cost_floor, which matters only where the
cost itself is rounding: the noiseless frames); the information against NumPy at the GPU's own pose and mask to
1e-12 of its largest diagonal entry (<= 1344 positive terms per sum in f64:
only the summation order differs)."""
import ctypes
import functools

import numpy as np
import pytest

import guided_ref as gr
import pose_refine_ref as pr

W, H = 640, 480
P3 = np.array([[500.0, 0, 320.0, 0], [0, 500.0, 240.0, 0], [0, 0, 1.0, 0]])
P4 = np.array([[500.0, 0, 320.0, -60.0], [0, 500.0, 240.0, 3.0], [0, 0, 1.0, 0.02]])
GATE = 2.4477
ROWS_CAP = 1344
# observations per frame: empty; below min_inliers (status 1); exactly min_inliers; a few
# lanes of one wave; a full wave and one more; one per lane and the wrap; beyond the
# register-held 1024; and one frame of garbage (status 2)
COUNTS = [0, 2, 3, 5, 64, 65, 256, 257, 1025, 1300, 40]
GARBAGE = 10
MIN_INL = 3
OPTS = dict(gate=GATE, min_depth=0.1, n_rounds=4, iters=10, min_inliers=MIN_INL)


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    return pr.rodrigues(a / np.linalg.norm(a) * angle)


def _pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def _project(P, Xc):
    h = Xc @ P[:, :3].T + P[:, 3]
    return h[:, :2] / h[:, 2:3]


def _angle(Ra, Rb):
    return np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0))


def _cost_floor(n, cost):
    """What rounding alone does to a cost of n observations: a residual component
    carries an error of at most d = 16 eps max(W, H) (a dozen operations on pixel
    values), so sum |r|^2 moves by at most 2 d sqrt(n cost) + n d^2.  On noisy
    frames that is 1e-12 of the cost, far below the 1e-8 bar; on the noiseless
    ones the cost itself is rounding (1e-26) and a relative bar alone means nothing."""
    d = 16 * np.finfo(np.float64).eps * max(W, H)
    return 2 * d * np.sqrt(n * cost) + n * d * d


def _frustum(rng, n):
    z = rng.uniform(4.0, 20.0, n)
    return np.stack([rng.uniform(-0.55, 0.55, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], 1)


# ----------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("w", [(0.0, 0.0, 0.0), (3e-14, -1e-14, 2e-14), (0.2, -0.15, 0.17)])
def test_reference_jacobian_against_central_differences(w):
    """Analytic 2x6 Jacobian of the reference against central differences of its own
    residual: step 1e-6 (truncation ~ h^2, rounding ~ eps |uv| / h ~ 1e-8 px on
    entries of ~ 1e3), relative error <= 1e-7; a P with a non-zero fourth column."""
    rng = np.random.default_rng(3)
    Q = _frustum(rng, 40)
    p = np.r_[w, 0.05, -0.03, 0.08]
    xy = _project(P4, Q @ pr.rodrigues(p[:3]).T + p[3:]) + rng.uniform(-2, 2, (40, 2))
    r, valid, J = pr.residual(p, Q, xy, P4, 0.1, jac=True)
    assert valid.all() and J.shape == (40, 2, 6)
    h = 1e-6
    fd = np.zeros_like(J)
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        fd[:, :, k] = (pr.residual(p + e, Q, xy, P4, 0.1)[0] - pr.residual(p - e, Q, xy, P4, 0.1)[0]) / (2 * h)
    err = np.abs(fd - J).max() / np.abs(J).max()
    print(f"|w| = {np.linalg.norm(w):.3g}: Jacobian relative error {err:.3g}")
    assert err <= 1e-7


@pytest.mark.parametrize("yaw", [0.0, 3.1])
def test_reference_recovers_true_pose_on_noiseless_data(yaw):
    rng = np.random.default_rng(4)
    true = _pose(_rot((0, 1, 0), yaw) @ _rot((1, 2, -1), 0.05), (0.3, -0.2, 0.5))
    pred = _pose(true[:3, :3] @ _rot((0.3, 1, 0.2), 0.004), true[:3, 3] + (0.08, -0.03, 0.05))
    assert abs(np.linalg.norm(pred[:3, 3] - true[:3, 3]) - 0.1) < 2e-3
    Xc = _frustum(rng, 60)
    X = Xc @ true[:3, :3].T + true[:3, 3]
    for P in (P3, P4):
        xy = _project(P, Xc)
        rows = np.c_[np.zeros(60), np.arange(60), xy]
        out = pr.refine(rows, 60, X, pred, P, loss=1, loss_scale=GATE, **OPTS)
        assert out["status"] == 0 and out["ninl"] == 60 and out["mask"].all()
        assert np.abs(out["pose"] - true).max() < 1e-9
        assert out["cost"] < 1e-15
        assert np.array_equal(out["info"], out["info"].T) and np.linalg.eigvalsh(out["info"]).min() > 0


def test_argument_errors_without_gpu():
    from slam355 import _lib

    L = _lib.lib
    err = lambda: L.slam_last_error()  # noqa: E731
    buf = (ctypes.c_double * 64)()       # never read: every call below is refused before any GPU call
    q = ctypes.c_void_p(ctypes.addressof(buf))

    def call(rows_cap=100, batch=2, n_x=10, loss=1, loss_scale=2.0, gate=2.0, n_rounds=4, iters=10,
             min_inliers=10, ptrs=(q,) * 11):
        rows, count, X, poses, P, po, mask, ninl, status, info, cost = ptrs
        return L.slam_pose_refine(rows, count, rows_cap, batch, X, n_x, poses, P, loss, loss_scale,
                                  gate, 0.1, n_rounds, iters, min_inliers, po, mask, ninl, status,
                                  info, cost, None)
    for k in range(11):
        assert call(ptrs=(q,) * k + (None,) + (q,) * (10 - k)) == -1 and b"null" in err(), k
    for bad in (0, 65536, -1):
        assert call(batch=bad) == -1 and b"batch" in err()
        assert call(rows_cap=bad) == -1 and b"rows_cap" in err()
    assert call(n_x=-1) == -1 and b"n_x" in err()
    for bad in (0, 9):
        assert call(n_rounds=bad) == -1 and b"n_rounds" in err()
    for bad in (0, 51):
        assert call(iters=bad) == -1 and b"iters" in err()
    assert call(min_inliers=2) == -1 and b"min_inliers" in err()
    for bad in (-1, 4):
        assert call(loss=bad) == -1 and b"loss" in err()
    for bad in (0.0, -1.0, float("nan")):
        assert call(loss_scale=bad) == -1 and b"loss_scale" in err()
        assert call(gate=bad) == -1 and b"gate" in err()
    assert call(loss=0, loss_scale=0.0, gate=-2.0) == -1 and b"gate" in err()   # linear: scale unused


# ----------------------------------------------------------------------------- scenes
@functools.lru_cache(maxsize=None)
def _scene(p4, yaw):
    """One batch: a frame per entry of COUNTS.  30 % gross outliers (50-200 px),
    landmarks behind the camera, one landmark index >= n_x, +-1.5 px uniform noise
    on the rest; the frames of 3 and 5 observations are noiseless; frame GARBAGE
    holds random pixels only.  Predictions are 0.1 m and 0.004 rad off."""
    rng = np.random.default_rng(77)
    P = P4 if p4 else P3
    B = len(COUNTS)
    rows = np.zeros((B, ROWS_CAP, 4))
    rows[..., 1] = -5.0                       # rows >= count must not be read as landmarks
    pred, true, Xs, base = np.zeros((B, 4, 4)), np.zeros((B, 4, 4)), [], 0
    kinds = []
    for b, n in enumerate(COUNTS):
        Rt = _rot((0, 1, 0), yaw + 0.03 * b) @ _rot(rng.normal(0, 1, 3), 0.04)
        true[b] = _pose(Rt, rng.uniform(-1, 1, 3))
        dt = rng.normal(0, 1, 3)
        pred[b] = _pose(Rt @ _rot(rng.normal(0, 1, 3), 0.004), true[b, :3, 3] + 0.1 * dt / np.linalg.norm(dt))
        Xc = _frustum(rng, n)
        kind = np.zeros(n, np.int64)          # 0 inlier, 1 gross outlier, 2 behind, 3 index >= n_x
        if b == GARBAGE:
            kind[:] = 1
        elif n >= 64:
            kind[rng.random(n) < 0.3] = 1
            kind[rng.permutation(n)[:4]] = 2
            kind[rng.integers(0, n)] = 3
        Xc[kind == 2, 2] *= -1.0
        xy = _project(P, Xc)
        if n >= 64:
            xy += rng.uniform(-1.5, 1.5, (n, 2))
        ang = rng.uniform(0, 2 * np.pi, n)
        off = rng.uniform(50, 200, n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
        xy[kind == 1] += off[kind == 1]
        if b == GARBAGE:
            xy = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1)
        Xs.append(Xc @ Rt.T + true[b, :3, 3])
        rows[b, :n] = np.c_[np.full(n, b), base + np.arange(n), xy]
        kinds.append(kind)
        base += n
    X = np.concatenate(Xs)
    for b, kind in enumerate(kinds):
        rows[b, :len(kind), 1][kind == 3] = len(X) + 5
    return dict(P=P, rows=rows, count=np.array(COUNTS, np.int32), X=X, pred=pred, true=true,
                kinds=kinds)


@functools.lru_cache(maxsize=None)
def _reference(p4, yaw, loss):
    s = _scene(p4, yaw)
    return [pr.refine(s["rows"][b], s["count"][b], s["X"], s["pred"][b], s["P"], loss=loss,
                      loss_scale=GATE, **OPTS) for b in range(len(COUNTS))]


CASES = [(p4, 0.0, loss) for p4 in (False, True) for loss in range(4)] + [(False, 3.1, 1), (True, 3.1, 1)]


@pytest.mark.parametrize("p4,yaw,loss", CASES)
def test_reference_on_the_scenes(p4, yaw, loss):
    """What the scenes are there to show, and the condition on the inputs: no |r|^2
    within a relative 1e-6 of gate^2 at any classification of the reference."""
    s, ref = _scene(p4, yaw), _reference(p4, yaw, loss)
    st = [o["status"] for o in ref]
    assert st[:2] == [1, 1] and st[GARBAGE] == 2
    assert min(o["margin"] for o in ref) > 1e-6
    for b in (2, 3):                              # noiseless: the true pose
        assert st[b] == 0 and ref[b]["ninl"] == COUNTS[b]
        assert np.abs(ref[b]["pose"] - s["true"][b]).max() < 1e-7
    if loss == 0:
        return                                    # the plain loss is at the mercy of the outliers
    for b in range(4, 10):
        o, kind = ref[b], s["kinds"][b]
        assert o["status"] == 0
        assert not o["mask"][kind != 0].any() and o["mask"][kind == 0].mean() > 0.9
        et = np.linalg.norm(o["pose"][:3, 3] - s["true"][b, :3, 3])
        assert et < 0.05 and _angle(o["pose"][:3, :3], s["true"][b, :3, :3]) < 2e-3
        assert et < np.linalg.norm(s["pred"][b, :3, 3] - s["true"][b, :3, 3])


# ----------------------------------------------------------------------------- GPU
def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("p4,yaw,loss", CASES)
def test_refine_pose_against_reference(p4, yaw, loss):
    import torch
    from slam355 import geometry

    s, ref = _scene(p4, yaw), _reference(p4, yaw, loss)
    B = len(COUNTS)
    assert min(o["margin"] for o in ref) > 1e-6   # the condition on the inputs
    X = _dev(s["X"])
    out = (torch.full((B, 4, 4), 9.0, dtype=torch.float64, device="cuda"),
           torch.full((B, ROWS_CAP), 7, dtype=torch.uint8, device="cuda"),
           torch.full((B,), 99, dtype=torch.int32, device="cuda"),
           torch.full((B,), 99, dtype=torch.int32, device="cuda"),
           torch.full((B, 6, 6), 9.0, dtype=torch.float64, device="cuda"),
           torch.full((B,), 9.0, dtype=torch.float64, device="cuda"))
    name = [k for k, v in geometry.REFINE_LOSSES.items() if v == loss][0]
    got = geometry.refine_pose(_dev(s["rows"]), _dev(s["count"]), X, len(s["X"]), _dev(s["pred"]),
                               s["P"], loss=name, loss_scale=GATE, gate=GATE, rounds=4, iters=10,
                               min_inliers=MIN_INL, min_depth=0.1, out=out)
    pose, mask, ninl, status, info, cost = (t.cpu().numpy() for t in got)
    for b, o in enumerate(ref):
        n = COUNTS[b]
        assert status[b] == o["status"] and ninl[b] == o["ninl"], (b, status[b], ninl[b], o["status"], o["ninl"])
        assert np.array_equal(mask[b, :n].astype(bool), o["mask"]), b
        assert (mask[b, n:] == 7).all(), b                    # entries >= count are not written
        assert np.array_equal(info[b], info[b].T), b          # symmetric bit for bit
        if o["status"] != 0:
            assert np.array_equal(pose[b].view(np.uint64), s["pred"][b].view(np.uint64)), b
            assert not info[b].any() and cost[b] == 0.0 and ninl[b] == -1
            continue
        dR = np.abs(pose[b, :3, :3] - o["pose"][:3, :3]).max()
        dt = np.abs(pose[b, :3, 3] - o["pose"][:3, 3]).max()
        dc = abs(cost[b] - o["cost"])
        want = pr.information_at(pose[b], mask[b, :n], s["rows"][b, :n], s["X"], s["P"], loss, GATE)
        di = np.abs(info[b] - want).max() / np.diag(want).max()
        print(f"frame {b} ({n} obs, {ninl[b]} inliers): dR {dR:.2e} dt {dt:.2e} "
              f"dcost {dc / max(o['cost'], 1e-300):.2e} dinfo {di:.2e}")
        assert np.array_equal(pose[b, 3], [0.0, 0.0, 0.0, 1.0])
        assert dR <= 1e-8 and dt <= 1e-8 * (1.0 + np.abs(o["pose"][:3, 3]).max()), b
        assert dc <= 1e-8 * o["cost"] + _cost_floor(n, o["cost"]), b
        assert di <= 1e-12, b


# ----------------------------------------------------------------------------- localize
def _flip(rng, d, nbits):
    bits = np.unpackbits(d, axis=-1)
    for row in bits.reshape(-1, 256):
        row[rng.choice(256, nbits, replace=False)] ^= 1
    return np.packbits(bits, axis=-1)


def _yaw_pose(x, yaw):
    T = np.eye(4)
    c, s = np.cos(yaw), np.sin(yaw)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[0, 3] = x
    return T


RADIUS = (15.0, 5.0)
LOC = dict(max_dist=64, ratio=(7, 10))


@functools.lru_cache(maxsize=None)
def _e2e_scene():
    """300 landmarks seen from four frames, keypoints +-1.5 px off their projections
    among 100 random ones; the poses handed to localize are 0.1 off in x and 0.004
    rad in yaw (predictions 10-11 px off)."""
    rng = np.random.default_rng(2024)
    nl, nf, cap = 300, 4, 448
    X = np.stack([rng.uniform(-6, 6, nl), rng.uniform(-4, 4, nl), rng.uniform(6, 20, nl)], 1)
    D = rng.integers(0, 256, (nl, 32), dtype=np.uint8)
    true = np.stack([_yaw_pose(0.4 * f, 0.02 * f) for f in range(nf)])
    pred = np.stack([_yaw_pose(0.4 * f + 0.1, 0.02 * f + 0.004) for f in range(nf)])
    kp = np.zeros((nf, cap, 5), np.float32)
    desc = np.zeros((nf, cap, 32), np.uint8)
    n_kp = np.zeros(nf, np.int32)
    truth = np.full((nf, cap), -1, np.int64)            # keypoint -> landmark
    for f in range(nf):
        uv, _ = gr.project(X, true[f], P3, W, H, 2.0, 0.1)    # noise of 1.5 px stays inside
        vis = np.nonzero(~np.isnan(uv[:, 0]))[0]
        pts = uv[vis].astype(np.float64) + rng.uniform(-1.5, 1.5, (len(vis), 2))
        des = _flip(rng, D[vis], 20)
        pts = np.r_[pts, np.stack([rng.uniform(0, W, 100), rng.uniform(0, H, 100)], 1)]
        des = np.r_[des, rng.integers(0, 256, (100, 32), dtype=np.uint8)]
        lm = np.r_[vis, np.full(100, -1)]
        order = rng.permutation(len(pts))
        m = len(pts)
        kp[f, :m, :2], desc[f, :m], truth[f, :m], n_kp[f] = pts[order], des[order], lm[order], m
    return dict(X=X, D=D, true=true, pred=pred, kp=kp, desc=desc, n_kp=n_kp, truth=truth, cap=cap,
                nl=nl, nf=nf)


def _match_ref(s, f, uv, radius):
    qr = np.full(s["nl"], radius, np.float32)
    i2, d2, g = gr.window_knn2(s["D"], uv, qr, s["desc"][f], s["kp"][f], s["n_kp"][f], W, H,
                               LOC["max_dist"], LOC["ratio"])
    _, good = gr.unique(i2, d2, g, s["cap"])
    return gr.track_rows(i2, good, s["kp"][f], f), i2


def _refine_ref(s, rows, pose):
    return pr.refine(rows, len(rows), s["X"], pose, P3, loss=1, loss_scale=GATE, gate=GATE,
                     min_depth=0.1, n_rounds=4, iters=10, min_inliers=10)


def _pose_close(a, b):
    return (np.abs(a[:3, :3] - b[:3, :3]).max() <= 1e-8 and
            np.abs(a[:3, 3] - b[:3, 3]).max() <= 1e-8 * (1.0 + np.abs(b[:3, 3]).max()))


def test_reference_chain_localizes():
    """The reference alone (projection, matching and refinement on the CPU) meets
    what the GPU test asks of the scene."""
    s = _e2e_scene()
    for f in range(s["nf"]):
        uv, _ = gr.project(s["X"], s["pred"][f], P3, W, H, 0.0, 0.1)
        rows, _ = _match_ref(s, f, uv, RADIUS[0])
        one = _refine_ref(s, rows, s["pred"][f])
        uv, _ = gr.project(s["X"], one["pose"], P3, W, H, 0.0, 0.1)
        rows, i2 = _match_ref(s, f, uv, RADIUS[1])
        two = _refine_ref(s, rows, one["pose"])
        assert one["status"] == 0 and two["status"] == 0 and min(one["margin"], two["margin"]) > 1e-6
        l = rows[:, 1].astype(int)
        assert len(rows) > 200 and np.array_equal(s["truth"][f, i2[l, 0]], l)
        T, T0, Tt = two["pose"], s["pred"][f], s["true"][f]
        assert np.linalg.norm(T[:3, 3] - Tt[:3, 3]) < np.linalg.norm(T0[:3, 3] - Tt[:3, 3])
        assert _angle(T[:3, :3], Tt[:3, :3]) < _angle(T0[:3, :3], Tt[:3, :3])


def _localize(s, lm=None):
    from slam355.mapping import LandmarkMap

    if lm is None:
        lm = LandmarkMap(s["nl"], s["cap"], W, H, P3).add(s["X"], s["D"])
    return lm, (_dev(s["pred"]), _dev(s["kp"]), _dev(s["desc"]), _dev(s["n_kp"]))


@pytest.mark.gpu
def test_localize_end_to_end():
    s = _e2e_scene()
    lm, args = _localize(s)
    # the first pass's projection: the same kernel on the same poses, kept aside
    lm.observe(0, *args, radius=RADIUS[0], **LOC)
    uv1 = lm.uv.cpu().numpy().copy()
    lm.reset_tracks()
    pose, rows, count, mask, ninl, status, info = lm.localize(0, *args, radius=RADIUS, **LOC)
    uv2 = lm.uv.cpu().numpy()
    first = [t.cpu().numpy() for t in lm.first]
    pose, rows, count, mask, ninl, status, info, cost = (
        t.cpu().numpy() for t in (pose, rows, count, mask, ninl, status, info, lm.cost))
    for f in range(s["nf"]):
        rows1, _ = _match_ref(s, f, uv1[f], RADIUS[0])
        one = _refine_ref(s, rows1, s["pred"][f])
        assert first[3][f] == one["status"] == 0 and first[2][f] == one["ninl"]
        assert np.array_equal(first[1][f, :len(rows1)].astype(bool), one["mask"])
        assert _pose_close(first[0][f], one["pose"]), f
        # second pass: the reference on the GPU's own uv and first pose
        rows2, i2 = _match_ref(s, f, uv2[f], RADIUS[1])
        assert count[f] == len(rows2) and np.array_equal(rows[f, :count[f]], rows2), f
        two = _refine_ref(s, rows2, first[0][f])
        assert min(one["margin"], two["margin"]) > 1e-6
        assert status[f] == two["status"] == 0 and ninl[f] == two["ninl"], f
        assert np.array_equal(mask[f, :count[f]].astype(bool), two["mask"]), f
        assert _pose_close(pose[f], two["pose"]), f
        assert abs(cost[f] - two["cost"]) <= 1e-8 * two["cost"] + _cost_floor(count[f], two["cost"]), f
        want = pr.information_at(pose[f], mask[f, :count[f]], rows2, s["X"], P3, 1, GATE)
        assert np.abs(info[f] - want).max() <= 1e-12 * np.diag(want).max(), f
        assert np.array_equal(info[f], info[f].T)
        # no wrong keypoint in the second pass, and the pose is closer than the prediction
        l = rows2[:, 1].astype(int)
        assert len(l) > 200 and np.array_equal(s["truth"][f, i2[l, 0]], l), f
        Tt, T0 = s["true"][f], s["pred"][f]
        et, et0 = np.linalg.norm(pose[f, :3, 3] - Tt[:3, 3]), np.linalg.norm(T0[:3, 3] - Tt[:3, 3])
        ea, ea0 = _angle(pose[f, :3, :3], Tt[:3, :3]), _angle(T0[:3, :3], Tt[:3, :3])
        print(f"frame {f}: {count[f]} rows, {ninl[f]} inliers, translation error {et0:.3f} -> {et:.4f}, "
              f"rotation error {ea0:.4f} -> {ea:.5f} rad")
        assert et < et0 and ea < ea0, f
    # only the second pass's rows are kept for tracks()
    om = lm.tracks()
    assert len(om) == count.sum() and np.array_equal(om[:count[0]], rows[0, :count[0]])


@pytest.mark.gpu
def test_localize_in_graph_capture():
    import torch

    s = _e2e_scene()
    lm, args = _localize(s)
    want = lm.localize(0, *args, radius=RADIUS, **LOC)     # eager; also allocates the buffers
    want = [t.cpu().numpy().copy() for t in want]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = lm.localize(0, *args, radius=RADIUS, **LOC)  # a host sync or a hipMalloc here fails the capture
    for t in got:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in got]
    count = got[2]
    assert np.array_equal(count, want[2]) and count.min() > 200
    assert (got[5] == 0).all() and np.array_equal(got[4], want[4])
    for f in range(s["nf"]):
        c = count[f]
        assert np.array_equal(got[1][f, :c], want[1][f, :c])
        assert np.array_equal(got[3][f, :c], want[3][f, :c])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[6], want[6])
