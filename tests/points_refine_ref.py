"""NumPy f64 restatement of slam_points_refine (include/slam355.h): the reference
of tests/test_points_refine.py.  One landmark at a time; the residuals and
Jacobians of a landmark's frames are formed elementwise (so every entry is the
scalar expression of the header, in its order), the sums over the frames are
explicit loops in frame order, and the 3x3 algebra is scalar."""
import numpy as np

LOSSES = {"linear": 0, "huber": 1, "soft_l1": 2, "cauchy": 3}
F = np.float64


def index_rows(rows, count, x_cap):
    """-> tab [n_frames, x_cap] int: the lowest k < count_f of frame f whose
    landmark column equals i exactly, -1 where there is none."""
    rows = np.asarray(rows, F)
    nf, rows_cap = rows.shape[:2]
    tab = np.full((nf, x_cap), -1, np.int64)
    for f in range(nf):
        c = min(max(int(count[f]), 0), rows_cap)
        for k in range(c - 1, -1, -1):          # descending: the lowest k is written last
            l = rows[f, k, 1]
            if l >= 0 and l < x_cap and float(int(l)) == l:
                tab[f, int(l)] = k
    return tab


def residual(T, xy, P, X, min_depth, jac=False):
    """T [m,4,4] poses, xy [m,2] pixels, X [3] -> r [m,2], valid [m] (and J [m,2,3]).
    Broadcast over the frames and the components only: every entry is the
    header's scalar expression, parenthesised left to right."""
    T = np.asarray(T, F).reshape(-1, 4, 4)
    P = np.asarray(P, F).reshape(3, 4)
    X = np.asarray(X, F)
    with np.errstate(all="ignore"):
        d = X[None, :] - T[:, :3, 3]
        Xc = (T[:, 0, :3] * d[:, 0:1] + T[:, 1, :3] * d[:, 1:2]) + T[:, 2, :3] * d[:, 2:3]
        h = ((P[None, :, 0] * Xc[:, 0:1] + P[None, :, 1] * Xc[:, 1:2]) + P[None, :, 2] * Xc[:, 2:3]) \
            + P[None, :, 3]
        iz = 1.0 / h[:, 2:3]
        uv = h[:, :2] * iz
        r = uv - xy
        valid = (Xc[:, 2] > min_depth) & (h[:, 2] > 0.0)
        if not jac:
            return r, valid
        a = (P[None, :2, :3] - uv[:, :, None] * P[None, 2:3, :3]) * iz[:, :, None]      # [m,2,3]
        R = T[:, None, :3, :3]                                                          # [m,1,k,j]
        J = (a[:, :, None, 0] * R[..., 0] + a[:, :, None, 1] * R[..., 1]) + a[:, :, None, 2] * R[..., 2]
        return r, valid, J


def robust(r, J, loss, delta):
    """robust_loss.hpp: -> (r, J scaled by sqrt(rho'), term = delta^2 rho); loss 0: |r|^2."""
    s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
    if loss == 0:
        return r, J, s
    d2 = delta * delta
    z = s / d2
    with np.errstate(all="ignore"):
        if loss == 1:
            q = np.sqrt(z)
            big = ~(z <= 1.0)
            sw = np.where(big, 1.0 / np.sqrt(q), 1.0)
            term = np.where(big, d2 * (2.0 * q - 1.0), s)
        elif loss == 2:
            q = np.sqrt(1.0 + z)
            sw = 1.0 / np.sqrt(q)
            term = d2 * (2.0 * z / (q + 1.0))
        else:
            sw = 1.0 / np.sqrt(1.0 + z)
            term = d2 * np.log1p(z)
        if loss == 1:       # huber below the knee: nothing is scaled (not even by 1.0)
            rs = np.where(big[:, None], r * sw[:, None], r)
            Js = None if J is None else np.where(big[:, None, None], J * sw[:, None, None], J)
        else:
            rs = r * sw[:, None]
            Js = None if J is None else J * sw[:, None, None]
    return rs, Js, term


def normal_sums(T, xy, P, X, min_depth, loss, delta):
    """H [3,3] (symmetric), g [3], cost over the given observations, in their
    order; per observation row 0 of J, then row 1."""
    r, _, J = residual(T, xy, P, X, min_depth, jac=True)
    r, J, term = robust(r, J, loss, delta)
    with np.errstate(all="ignore"):
        V = np.concatenate([(J[:, :, :, None] * J[:, :, None, :]).reshape(-1, 2, 9),
                            J * r[:, :, None]], 2).reshape(-1, 12)
        acc, cost = np.zeros(12), 0.0
        for row in V:
            acc = acc + row
        for v in term.tolist():
            cost = cost + v
    return acc[:9].reshape(3, 3), acc[9:], cost


def solve3(H, g, lam):
    """(H + lam max(diag H, 1e-12)) d = -g by Cholesky, scalar; None on failure."""
    with np.errstate(all="ignore"):
        a00 = H[0, 0] + lam * max(H[0, 0], 1e-12)
        a11 = H[1, 1] + lam * max(H[1, 1], 1e-12)
        a22 = H[2, 2] + lam * max(H[2, 2], 1e-12)
        if not a00 > 0.0:
            return None
        l00 = np.sqrt(a00)
        l10, l20 = H[1, 0] / l00, H[2, 0] / l00
        s1 = a11 - l10 * l10
        if not s1 > 0.0:
            return None
        l11 = np.sqrt(s1)
        l21 = (H[2, 1] - l20 * l10) / l11
        s2 = (a22 - l20 * l20) - l21 * l21
        if not s2 > 0.0:
            return None
        l22 = np.sqrt(s2)
        y0 = -g[0] / l00
        y1 = (-g[1] - l10 * y0) / l11
        y2 = ((-g[2] - l20 * y0) - l21 * y1) / l22
        d2 = y2 / l22
        d1 = (y1 - l21 * d2) / l11
        d0 = ((y0 - l10 * d1) - l20 * d2) / l00
    return np.array([d0, d1, d2])


def max_variance(H):
    """The largest diagonal entry of H^-1 through H = L L^T, M = L^-1; None when a
    pivot is not positive and finite."""
    with np.errstate(all="ignore"):
        if not (H[0, 0] > 0.0 and H[0, 0] < np.inf):
            return None
        l00 = np.sqrt(H[0, 0])
        l10, l20 = H[1, 0] / l00, H[2, 0] / l00
        s1 = H[1, 1] - l10 * l10
        if not (s1 > 0.0 and s1 < np.inf):
            return None
        l11 = np.sqrt(s1)
        l21 = (H[2, 1] - l20 * l10) / l11
        s2 = (H[2, 2] - l20 * l20) - l21 * l21
        if not (s2 > 0.0 and s2 < np.inf):
            return None
        l22 = np.sqrt(s2)
        m00, m11, m22 = 1.0 / l00, 1.0 / l11, 1.0 / l22
        m10 = -(l10 * m00) / l11
        m21 = -(l21 * m11) / l22
        m20 = -(l20 * m00 + l21 * m10) / l22
        v0 = (m00 * m00 + m10 * m10) + m20 * m20
        v1 = m11 * m11 + m21 * m21
        v2 = m22 * m22
    return max(v0, max(v1, v2))


def refine_one(T, xy, P, X, loss=1, loss_scale=2.4477, gate=2.4477, min_depth=0.1, n_rounds=3,
               iters=8, min_obs=3, max_var=0.25):
    """One landmark from its observations in frame order: T [m,4,4], xy [m,2], X [3].
    -> dict(X, status, nobs, cost, info, var, inl [m] bool, margin)."""
    T = np.asarray(T, F).reshape(-1, 4, 4)
    xy = np.asarray(xy, F).reshape(-1, 2)
    X0 = np.asarray(X, F).copy()
    m = len(T)
    none = dict(X=X0, nobs=-1, cost=0.0, info=np.zeros((3, 3)), var=0.0, margin=np.inf)
    if np.isnan(X0[0]):
        return dict(none, status=4, inl=np.zeros(m, bool))
    gate2 = gate * gate
    margin = np.inf
    _, A = residual(T, xy, P, X0, min_depth)
    if A.sum() < min_obs:
        return dict(none, status=1, inl=A)
    Xk = X0.copy()
    for _ in range(n_rounds):
        lam = 1e-3
        for _ in range(iters):
            H, g, cost = normal_sums(T[A], xy[A], P, Xk, min_depth, loss, loss_scale)
            d = solve3(H, g, lam)
            ok = d is not None
            if ok:
                Xn = Xk + d
                rt, vt = residual(T[A], xy[A], P, Xn, min_depth)
                term = robust(rt, None, loss, loss_scale)[2]
                cn = F(0.0)
                with np.errstate(all="ignore"):
                    for v in term:
                        cn = cn + v
                ok = bool(vt.all()) and bool(cn < cost)
            if ok:
                Xk = Xn
                lam = max(lam * 0.1, 1e-12)
            else:
                lam = min(lam * 10.0, 1e12)
        r, v = residual(T, xy, P, Xk, min_depth)
        with np.errstate(all="ignore"):
            s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
            if v.any():
                margin = min(margin, np.abs(s[v] - gate2).min() / gate2)
            A = v & (s <= gate2)
        if A.sum() < min_obs:
            return dict(none, status=2, inl=A, margin=margin)
    H, _, cost = normal_sums(T[A], xy[A], P, Xk, min_depth, loss, loss_scale)
    var = max_variance(H)
    if var is None:
        status, var = 3, np.inf
    else:
        status = 0 if var <= max_var else 3
        if np.isfinite(max_var):
            margin = min(margin, abs(var - max_var) / max_var)
    return dict(X=Xk if status == 0 else X0, status=status, nobs=int(A.sum()), cost=float(cost),
                info=H, var=float(var), inl=A, margin=margin)


def refine(rows, count, poses, P, X, n, kill=False, **opts):
    """The whole call.  rows [n_frames,rows_cap,4], count [n_frames], poses
    [n_frames,4,4], X [x_cap,3], n the landmark count -> dict(X, status, nobs,
    cost, info, var [x_cap...], mask [n_frames,rows_cap] u8 (entries >= count are
    0 here and not written on the device), nkilled, margin [x_cap])."""
    rows = np.asarray(rows, F)
    poses = np.asarray(poses, F).reshape(-1, 4, 4)
    X = np.asarray(X, F).copy()
    nf, rows_cap = rows.shape[:2]
    x_cap = len(X)
    n = min(max(int(n), 0), x_cap)
    tab = index_rows(rows, count, x_cap)
    out = dict(X=X, status=np.full(x_cap, -1, np.int32), nobs=np.full(x_cap, -1, np.int32),
               cost=np.zeros(x_cap), info=np.zeros((x_cap, 3, 3)), var=np.zeros(x_cap),
               mask=np.zeros((nf, rows_cap), np.uint8), nkilled=0, margin=np.full(x_cap, np.inf))
    for i in range(n):
        fr = np.nonzero(tab[:, i] >= 0)[0]
        k = tab[fr, i]
        o = refine_one(poses[fr], rows[fr, k, 2:4], P, X[i], **opts)
        out["status"][i], out["nobs"][i], out["cost"][i] = o["status"], o["nobs"], o["cost"]
        out["info"][i], out["var"][i], out["margin"][i] = o["info"], o["var"], o["margin"]
        out["mask"][fr, k] = o["inl"]
        X[i] = o["X"]
        if kill and o["status"] == 2:
            X[i] = np.nan
            out["nkilled"] += 1
    return out
