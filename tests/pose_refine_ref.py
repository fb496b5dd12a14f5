"""NumPy f64 restatement of slam_pose_refine (include/slam355.h): the reference
of tests/test_pose_refine.py.  Vectorised over the observations of one frame;
sums are NumPy's, so results differ from the kernel's by summation order only."""
import numpy as np

LOSSES = {"linear": 0, "huber": 1, "soft_l1": 2, "cauchy": 3}


def skew(a):
    """[a]x for a [...,3] -> [...,3,3]."""
    a = np.asarray(a, np.float64)
    z = np.zeros(a.shape[:-1])
    return np.stack([np.stack([z, -a[..., 2], a[..., 1]], -1),
                     np.stack([a[..., 2], z, -a[..., 0]], -1),
                     np.stack([-a[..., 1], a[..., 0], z], -1)], -2)


def rodrigues(w):
    """cv::Rodrigues, identity below |w| = 2^-52."""
    w = np.asarray(w, np.float64)
    th = np.sqrt(w @ w)
    if th < 2.220446049250313e-16:
        return np.eye(3)
    k = w / th
    return np.cos(th) * np.eye(3) + (1.0 - np.cos(th)) * np.outer(k, k) + np.sin(th) * skew(k)


def frame_points(rows, X, pose):
    """-> (Q [n,3] = R^T (X_l - t), xy [n,2], landmark-in-map [n])."""
    rows = np.asarray(rows, np.float64).reshape(-1, 4)
    X = np.asarray(X, np.float64).reshape(-1, 3)
    l = rows[:, 1]
    ok = (l >= 0) & (l < len(X))
    li = np.where(ok, l, 0).astype(np.int64)
    Xl = X[li] if len(X) else np.zeros((len(rows), 3))
    Xl = np.where(ok[:, None], Xl, 0.0)
    T = np.asarray(pose, np.float64).reshape(4, 4)
    return (Xl - T[:3, 3]) @ T[:3, :3], rows[:, 2:4].copy(), ok


def residual(p, Q, xy, P, min_depth, jac=False):
    """r [n,2], valid [n] (and J [n,2,6]) at the left increment p = (w, v)."""
    p = np.asarray(p, np.float64)
    P = np.asarray(P, np.float64).reshape(3, 4)
    R = rodrigues(p[:3])
    RQ = Q @ R.T
    Xc = RQ + p[3:]
    h = Xc @ P[:, :3].T + P[:, 3]
    with np.errstate(all="ignore"):
        iz = 1.0 / h[:, 2]
        uv = h[:, :2] * iz[:, None]
        r = uv - xy
        valid = (Xc[:, 2] > min_depth) & (h[:, 2] > 0.0)
        if not jac:
            return r, valid
        a = (P[None, :2, :3] - uv[:, :, None] * P[None, 2:3, :3]) * iz[:, None, None]   # [n,2,3]
        w = p[:3]
        th2 = w @ w
        if th2 < 1e-24:
            D = -skew(RQ)
        else:
            Am = np.outer(w, w) + (R.T - np.eye(3)) @ skew(w)
            D = -(R @ skew(Q) @ Am) / th2
        return r, valid, np.concatenate([a @ D, a], -1)


def robust(r, J, loss, delta):
    """-> (r, J scaled by sqrt(rho'), term = delta^2 rho) per observation; loss 0: |r|^2."""
    s = (r * r).sum(1)
    if loss == 0:
        return r, J, s
    d2 = delta * delta
    z = s / d2
    with np.errstate(all="ignore"):
        if loss == 1:
            q = np.sqrt(z)
            big = z > 1.0
            sw = np.where(big, 1.0 / np.sqrt(q), 1.0)
            term = np.where(big, d2 * (2.0 * q - 1.0), s)
        elif loss == 2:
            q = np.sqrt(1.0 + z)
            sw = 1.0 / np.sqrt(q)
            term = d2 * (2.0 * z / (q + 1.0))
        else:
            sw = 1.0 / np.sqrt(1.0 + z)
            term = d2 * np.log1p(z)
    return r * sw[:, None], (None if J is None else J * sw[:, None, None]), term


def solve6(H, g, lam):
    A = H + lam * np.diag(np.maximum(np.diag(H), 1e-12))
    if not np.isfinite(A).all():
        return None
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    return -np.linalg.solve(L.T, np.linalg.solve(L, g))


def pose_out(pose, p):
    T = np.asarray(pose, np.float64).reshape(4, 4)
    out = np.eye(4)
    out[:3, :3] = T[:3, :3] @ rodrigues(p[:3]).T
    out[:3, 3] = T[:3, 3] - out[:3, :3] @ p[3:]
    return out


def information(Xc, xy, P, loss, delta, min_depth=0.1):
    """sum J~^T J~ (and the robust cost) of the camera points Xc at increment 0."""
    r, _, J = residual(np.zeros(6), Xc, xy, P, min_depth, jac=True)
    r, J, term = robust(r, J, loss, delta)
    Jf = J.reshape(-1, 6)
    return Jf.T @ Jf, term.sum()


def information_at(pose, mask, rows, X, P, loss, delta):
    """The information at a given (returned) pose over a given mask."""
    Q, xy, _ = frame_points(rows, X, pose)
    m = np.asarray(mask).astype(bool)
    return information(Q[m], xy[m], P, loss, delta)[0]


def refine(rows, count, X, pose, P, loss=1, loss_scale=2.4477, gate=2.4477, min_depth=0.1,
           n_rounds=4, iters=10, min_inliers=10):
    """One frame.  -> dict(pose, mask, ninl, status, info, cost, margin, p) where
    margin is the smallest relative distance | |r|^2 - gate^2 | / gate^2 met at any
    classification (over the observations valid there)."""
    n = int(count)
    Q, xy, lok = frame_points(np.asarray(rows)[:n], X, pose)
    gate2 = gate * gate
    p = np.zeros(6)
    margin = [np.inf]

    def classify(gated):
        r, v = residual(p, Q, xy, P, min_depth)
        v &= lok
        if not gated:
            return v
        with np.errstate(all="ignore"):
            s = (r * r).sum(1)
            if v.any():
                margin[0] = min(margin[0], np.abs(s[v] - gate2).min() / gate2)
            return v & (s <= gate2)

    fail = dict(pose=np.asarray(pose, np.float64).reshape(4, 4).copy(), ninl=-1, info=np.zeros((6, 6)),
                cost=0.0)
    A = classify(False)
    if A.sum() < min_inliers:
        return dict(fail, mask=A, status=1, margin=margin[0], p=p)
    for _ in range(n_rounds):
        lam = 1e-3
        for _ in range(iters):
            r, _, J = residual(p, Q[A], xy[A], P, min_depth, jac=True)
            r, J, term = robust(r, J, loss, loss_scale)
            Jf = J.reshape(-1, 6)
            d = solve6(Jf.T @ Jf, Jf.T @ r.reshape(-1), lam)
            ok = d is not None
            if ok:
                rt, vt = residual(p + d, Q[A], xy[A], P, min_depth)
                ct = robust(rt, None, loss, loss_scale)[2].sum()
                ok = bool(vt.all()) and ct < term.sum()
            if ok:
                p = p + d
                lam = max(lam * 0.1, 1e-12)
            else:
                lam = min(lam * 10.0, 1e12)
        A = classify(True)
        if A.sum() < min_inliers:
            return dict(fail, mask=A, status=2, margin=margin[0], p=p)
    Xc = Q[A] @ rodrigues(p[:3]).T + p[3:]
    info, cost = information(Xc, xy[A], P, loss, loss_scale, min_depth)
    return dict(pose=pose_out(pose, p), mask=A, ninl=int(A.sum()), status=0, info=info, cost=cost,
                margin=margin[0], p=p)
