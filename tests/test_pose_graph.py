"""SE(3) pose graph (slam_pg_*, slam355.posegraph.PoseGraph / pg_schedule /
relative_pose / edges_from_ba).

Semantics (include/slam355.h): poses x_i = [r, t], T_i = [R(r_i) | t_i]; edge
k = (i, j, z_k, A_k) measures T_i^-1 T_j; E = Z^-1 T_i^-1 T_j, e_k = [Log(R_E);
t_E], r_k = A_k e_k; held columns leave the Jacobian; the robust weight is the
BA's on s = |r_k|^2; the LM iteration is oracle.ba.lm_iteration's on H = J~^T
J~, g = -J~^T r~, D = clip(diag H, 1e-6, 1e32).

Reference: the NumPy restatement below (edge residual, closed-form Jacobian,
dense H and g, the LM iteration with np.linalg.solve, the robust weights).  It
is checked here on the CPU against central differences and against
scipy.optimize.least_squares before anything on the GPU is compared with it.

Bars (float64): residuals and Jacobians 1e-9 relative (the BA residual bar);
LM iterates those of test_gpu_tiled_solver_iterates_match_oracle: parameters
rtol 1e-6 + atol 1e-9, COST_NEW 1e-8 relative, lambda 1e-6 relative, ACCEPTED,
NACCEPT and CHOL_FAIL equal.  Conditions on the reference alone, asserted
before any comparison: in every compared iteration |cost - cost_new| >= 1e-6
cost (no accept flag is decided by rounding); every edge's residual angle at
the live and the trial point is < pi - 0.05; start (b) holds a rejection and
an acceptance; the steps by np.linalg.solve and by Cholesky differ by <= 0.01
bar.

Graphs: the smallest at which each mechanism can go wrong -- N = 4 (one tile,
24 of 64 rows, an edge with i > j), N = 12 (two tiles, one pose alone in the
second), N = 35 chain (four tiles, tile-tridiagonal: skipped tiles in the
skyline), N = 35 with loops (a full last tile row, fill inside the profile, a
repeated pair, a trailing update with I > J > k; its profile is the full lower
triangle), N = 45 with one loop edge from tile 1 to tile 3 (a partial profile
with fill inside it and an update pair I > J > k).  Starts: the odometry start
plus N(0, 0.6) (a: 5 iterations) or N(0, 1.0) (b: 10 iterations) on the free
parameters, lambda0 = 1e-9, pose 0 held whole.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ba as oba

PI_MARGIN = 0.05
LAM0 = 1e-9
SMALL = 0.05  # below: the series of the SO(3) coefficients (as the kernels)
# f_scale of the robust runs: the measurement noise (sigma 0.01 per component)
# through A (rows of norm 2..3) gives inlier |r| of 0.05..0.1; 0.2 is two to
# three of them.  (At 1.5 the two wrong loop edges, spread over the chain by the
# linear solution, are inliers: |r| <= 0.53.)
ROBUST_DELTA = 0.2


# ----------------------------------------------------------------------------- restatement
def _abc(t2):
    if t2 < SMALL * SMALL:
        return (1.0 - t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0)),
                0.5 - t2 / 24.0 * (1.0 - t2 / 30.0 * (1.0 - t2 / 56.0)),
                1.0 / 6.0 - t2 / 120.0 * (1.0 - t2 / 42.0 * (1.0 - t2 / 72.0)))
    th = np.sqrt(t2)
    return np.sin(th) / th, 2.0 * np.sin(0.5 * th) ** 2 / t2, (th - np.sin(th)) / (t2 * th)


def _k(t2):
    if t2 < SMALL * SMALL:
        return 1.0 / 12.0 + t2 / 720.0 * (1.0 + t2 / 42.0 * (1.0 + t2 / 40.0))
    th = np.sqrt(t2)
    return (1.0 - 0.5 * th * np.cos(0.5 * th) / np.sin(0.5 * th)) / t2


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _poly(r, p, q):
    K = hat(r)
    return np.eye(3) + p * K + q * (np.outer(r, r) - float(r @ r) * np.eye(3))


def so3_exp(r):
    a, b, _ = _abc(float(r @ r))
    return _poly(r, a, b)


def so3_jr(r):
    _, b, c = _abc(float(r @ r))
    return _poly(r, -b, c)


def so3_jr_inv(r):
    return _poly(r, 0.5, _k(float(r @ r)))


def so3_log(R):
    """Rotation vector with angle in [0, pi]."""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s2 = float(v @ v)
    s, c = np.sqrt(s2), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, c)
    if c < 0.0 and s < 1e-3:  # within 1e-3 of pi: the axis from the symmetric part
        n = np.sqrt(np.maximum((np.diag(R) - c) / (1.0 - c), 0.0))
        m = int(np.argmax(n))
        for q in range(3):
            if q != m and R[m, q] + R[q, m] < 0.0:
                n[q] = -n[q]
        return (th if v @ n >= 0.0 else -th) * n
    if c > 0.0 and s < SMALL:
        f = 1.0 + s2 / 6.0 * (1.0 + s2 * 9.0 / 20.0 * (1.0 + s2 * 25.0 / 42.0))
    else:
        f = th / s
    return f * v


def edge_error(xi, xj, z):
    """e = [Log(R_z^T R_i^T R_j); R_z^T (R_i^T (t_j - t_i) - t_z)]."""
    Ri, Rj, Rz = so3_exp(xi[:3]), so3_exp(xj[:3]), so3_exp(z[:3])
    u = Ri.T @ (xj[3:] - xi[3:])
    return np.concatenate([so3_log(Rz.T @ (Ri.T @ Rj)), Rz.T @ (u - z[3:])])


def relative_pose(xi, xj):
    return edge_error(xi, xj, np.zeros(6))


def compose(xi, z):
    """x_j with relative_pose(x_i, x_j) = z."""
    Ri = so3_exp(xi[:3])
    return np.concatenate([so3_log(Ri @ so3_exp(z[:3])), xi[3:] + Ri @ z[3:]])


def edge_jacobian(xi, xj, z):
    """(e, d e / d x_i, d e / d x_j), the closed form of DESIGN.md 4d."""
    Ri, Rj, Rz = so3_exp(xi[:3]), so3_exp(xj[:3]), so3_exp(z[:3])
    u = Ri.T @ (xj[3:] - xi[3:])
    e = np.concatenate([so3_log(Rz.T @ (Ri.T @ Rj)), Rz.T @ (u - z[3:])])
    Jinv, Jri, Jrj = so3_jr_inv(e[:3]), so3_jr(xi[:3]), so3_jr(xj[:3])
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    Jj[:3, :3] = Jinv @ Jrj
    Ji[:3, :3] = -Jinv @ (Rj.T @ Ri @ Jri)
    Ji[3:, :3] = Rz.T @ hat(u) @ Jri
    Jj[3:, 3:] = Rz.T @ Ri.T
    Ji[3:, 3:] = -Jj[3:, 3:]
    return e, Ji, Jj


def rho_w(z, loss):
    """rho(z), w = rho'(z) of scipy's losses (tests/test_ba_loss.py)."""
    if loss == "linear":
        return z, 1.0
    if loss == "huber":
        return (2.0 * np.sqrt(z) - 1.0, 1.0 / np.sqrt(z)) if z > 1.0 else (z, 1.0)
    if loss == "soft_l1":
        return 2.0 * (np.sqrt(1.0 + z) - 1.0), 1.0 / np.sqrt(1.0 + z)
    if loss == "cauchy":
        return np.log1p(z), 1.0 / (1.0 + z)
    raise ValueError(loss)


def held_mask(words, N):
    if words is None:
        return np.zeros((N, 6), bool)
    return ((np.asarray(words, np.uint32)[:, None] >> np.arange(6, dtype=np.uint32)) & 1).astype(bool)


def graph_rj(x, edges, meas, A, words=None, loss="linear", delta=1.0, jac=True):
    """(raw e [E,6], r~ [E,6], J~_i, J~_j [E,6,6], cost terms d^2 rho(z) [E])."""
    E = len(edges)
    held = held_mask(words, len(x))
    e, rt, ct = np.zeros((E, 6)), np.zeros((E, 6)), np.zeros(E)
    Ji, Jj = np.zeros((E, 6, 6)), np.zeros((E, 6, 6))
    for k, (i, j) in enumerate(edges):
        if jac:
            e[k], a, b = edge_jacobian(x[i], x[j], meas[k])
            a[:, held[i]] = 0.0
            b[:, held[j]] = 0.0
            Ji[k], Jj[k] = A[k] @ a, A[k] @ b
        else:
            e[k] = edge_error(x[i], x[j], meas[k])
        rt[k] = A[k] @ e[k]
        s = float(rt[k] @ rt[k])
        rho, w = rho_w(s / delta ** 2, loss)
        ct[k] = s if loss == "linear" else delta ** 2 * rho
        sw = np.sqrt(w)
        rt[k] *= sw
        Ji[k] *= sw
        Jj[k] *= sw
    return e, rt, Ji, Jj, ct


def graph_cost(x, edges, meas, A, loss="linear", delta=1.0):
    return 0.5 * float(np.sum(graph_rj(x, edges, meas, A, None, loss, delta, jac=False)[4]))


def dense_system(x, edges, meas, A, words=None, loss="linear", delta=1.0):
    """Dense H = J~^T J~, g = -J~^T r~, cost, and the dense J~."""
    N, E = len(x), len(edges)
    _, rt, Ji, Jj, ct = graph_rj(x, edges, meas, A, words, loss, delta)
    Jd = np.zeros((6 * E, 6 * N))
    for k, (i, j) in enumerate(edges):
        Jd[6 * k:6 * k + 6, 6 * i:6 * i + 6] = Ji[k]
        Jd[6 * k:6 * k + 6, 6 * j:6 * j + 6] = Jj[k]
    return Jd.T @ Jd, -Jd.T @ rt.ravel(), 0.5 * float(ct.sum()), Jd


def max_angle(x, edges, meas):
    return max(float(np.linalg.norm(edge_error(x[i], x[j], meas[k])[:3])) for k, (i, j) in enumerate(edges))


def lm_iteration(x, edges, meas, A, st, words=None, loss="linear", delta=1.0):
    """oracle.ba.lm_iteration word for word on the pose graph's system.
    info adds the Cholesky route's step (a condition of the tests)."""
    H, g, cost, _ = dense_system(x, edges, meas, A, words, loss, delta)
    D = np.clip(np.diag(H), oba.DIAG_MIN, oba.DIAG_MAX)
    Hd = H + st.lam * np.diag(D)
    d = np.linalg.solve(Hd, g)
    try:
        Lc = np.linalg.cholesky(Hd)
        d_chol = np.linalg.solve(Lc.T, np.linalg.solve(Lc, g))
    except np.linalg.LinAlgError:
        d_chol = None
    xn = x + d.reshape(-1, 6)
    cost_new = graph_cost(xn, edges, meas, A, loss, delta)
    pred = 0.5 * float(d @ (st.lam * D * d + g))
    rho = (cost - cost_new) / pred if pred > 0 else -1.0
    accepted = rho > 0
    info = dict(cost=cost, cost_new=cost_new, pred=pred, rho=rho, accepted=accepted, lam_in=st.lam,
                delta=d, delta_chol=d_chol, x_trial=xn)
    if accepted:
        st.lam = min(max(st.lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), oba.LAM_MIN), oba.LAM_MAX)
        st.nu = 2.0
        x = xn
    else:
        st.lam = min(st.lam * st.nu, oba.LAM_MAX)
        st.nu *= 2.0
    return x, info


# ----------------------------------------------------------------------------- inputs
GRAPHS = {
    "n4": (4, [(0, 3), (3, 1)]),
    "n12": (12, [(0, 11), (2, 9)]),
    "n35chain": (35, []),
    "n35loops": (35, [(0, 34), (3, 27), (3, 27), (30, 5)]),
    # five tiles, one loop edge from tile 1 to tile 3: a partial profile (first = 0 0 1 1 3, 10 of
    # 15 tiles) with fill inside it and the update pair (3, 2) of column 1 (I > J > k)
    "n45loop": (45, [(12, 38)]),
}
# start seeds chosen on the CPU so that the conditions of the module docstring hold
SEEDS = {("n4", "a"): 3, ("n4", "b"): 4, ("n12", "a"): 1, ("n12", "b"): 1,
         ("n35chain", "a"): 7, ("n35chain", "b"): 1, ("n35loops", "a"): 1, ("n35loops", "b"): 9,
         ("n12", "r"): 1, ("n45loop", "b"): 11}
STARTS = {"a": (0.6, 5), "b": (1.0, 10), "r": (0.3, 4)}  # "r": the robust runs' start (sigma, iterations)


def truth(N):
    i = np.arange(N, dtype=np.float64)
    x = np.zeros((N, 6))
    x[:, 0] = 0.15 * np.sin(0.35 * i)
    x[:, 1] = 0.09 * i * (2.0 * np.pi / max(N, 12))
    x[:, 2] = 0.1 * np.cos(0.2 * i)
    x[:, 3] = 4.0 * np.cos(2.0 * np.pi * i / N)
    x[:, 4] = 4.0 * np.sin(2.0 * np.pi * i / N)
    x[:, 5] = 0.3 * np.sin(0.5 * i)
    return x


@functools.lru_cache(maxsize=None)
def graph(name, noise=0.01):
    """(truth, edges int32 [E,2], meas, information, A (upper factor), odometry
    start), shared and never written.  noise: sigma of the measurement noise."""
    N, loops = GRAPHS[name]
    rng = np.random.default_rng(11)
    xt = truth(N)
    edges = np.array([(i, i + 1) for i in range(N - 1)] + loops, np.int32)
    meas = np.stack([relative_pose(xt[i], xt[j]) for i, j in edges])
    meas = meas + rng.normal(0, noise, meas.shape)
    M = rng.normal(0, 1.0, (len(edges), 6, 6))
    info = 4.0 * np.eye(6) + 0.5 * M @ M.transpose(0, 2, 1)
    A = np.stack([np.linalg.cholesky(m).T for m in info])
    odo = np.zeros((N, 6))
    odo[0] = xt[0]
    for i in range(N - 1):
        odo[i + 1] = compose(odo[i], meas[i])
    for a in (xt, edges, meas, info, A, odo):
        a.setflags(write=False)
    return xt, edges, meas, info, A, odo


def fixed_words(N, extra=None):
    w = np.zeros(N, np.uint32)
    w[0] = 0x3F
    if extra is not None:
        w[extra[0]] = extra[1]
    return w


def start_of(name, which, words=None):
    sigma, _ = STARTS[which]
    xt, edges, meas, info, A, odo = graph(name)
    words = fixed_words(len(xt)) if words is None else words
    rng = np.random.default_rng(SEEDS[(name, which)])
    x0 = odo + rng.normal(0, sigma, odo.shape) * ~held_mask(words, len(xt))
    return x0


@functools.lru_cache(maxsize=None)
def reference_run(name, which, loss="linear", delta=1.0, wrong=False):
    """The restatement's iterates from start `which`: (x0, [info...], x_final).
    Asserts the module docstring's conditions on the reference."""
    xt, edges, meas, info, A, odo = graph(name)
    if wrong:
        meas = wrong_meas(name)
    words = fixed_words(len(xt))
    x0 = start_of(name, which)
    st = oba.LMState(LAM0)
    x, infos = x0.copy(), []
    for _ in range(STARTS[which][1]):
        assert max_angle(x, edges, meas) < np.pi - PI_MARGIN
        x, inf = lm_iteration(x, edges, meas, A, st, words, loss, delta)
        assert abs(inf["cost"] - inf["cost_new"]) >= 1e-6 * inf["cost"], (name, which, inf["cost"], inf["cost_new"])
        assert max_angle(inf["x_trial"], edges, meas) < np.pi - PI_MARGIN
        bar = 1e-6 * np.abs(inf["x_trial"].ravel()) + 1e-9
        assert inf["delta_chol"] is not None and np.all(np.abs(inf["delta"] - inf["delta_chol"]) <= 0.01 * bar)
        inf["lam_out"], inf["x_out"] = st.lam, x.copy()
        infos.append(inf)
    if which == "b":
        acc = [i["accepted"] for i in infos]
        assert any(acc) and not all(acc), acc
    return x0, infos, x


def wrong_meas(name):
    """Two loop edges measured wrong: off by 2 m and 0.5 rad."""
    xt, edges, meas, info, A, odo = graph(name)
    m = meas.copy()
    m[-1, 3] += 2.0
    m[-2, 1] += 0.5
    m.setflags(write=False)
    return m


# ----------------------------------------------------------------------------- CPU: the restatement
def _num_jac(xi, xj, z, h=1e-6):
    Ji, Jj = np.zeros((6, 6)), np.zeros((6, 6))
    for c in range(6):
        d = np.zeros(6)
        d[c] = h
        Ji[:, c] = (edge_error(xi + d, xj, z) - edge_error(xi - d, xj, z)) / (2 * h)
        Jj[:, c] = (edge_error(xi, xj + d, z) - edge_error(xi, xj - d, z)) / (2 * h)
    return Ji, Jj


@pytest.mark.parametrize("angle", [0.0, 1e-9, 1e-4, 0.04, 0.06, 1.0, 3.0])
def test_restatement_jacobian_against_central_differences(angle):
    """e = 0 exactly, the series / closed-form switch on both sides, and 3.0 rad."""
    rng = np.random.default_rng(5)
    for trial in range(4):
        xi = np.concatenate([rng.normal(0, 0.7, 3), rng.normal(0, 2.0, 3)])
        if trial == 3:
            xi[:3] *= 1e-3 / np.linalg.norm(xi[:3])  # a pose whose own rotation takes the series
        z = np.concatenate([rng.normal(0, 0.5, 3), rng.normal(0, 1.0, 3)])
        ax = rng.normal(0, 1, 3)
        off = np.concatenate([angle * ax / np.linalg.norm(ax), (0.0 if angle == 0.0 else 0.3) * rng.normal(0, 1, 3)])
        # x_j = x_i o z o off: then e = off up to rounding
        xj = compose(compose(xi, z), off)
        if angle == 0.0 and trial < 2:
            xj, z = xi.copy(), np.zeros(6)  # e = 0 exactly (R^T R is exactly symmetric)
            assert np.all(edge_error(xi, xj, z) == 0.0)
        elif angle == 0.0:
            z = relative_pose(xi, xj)  # e = 0 up to rounding
        e, Ji, Jj = edge_jacobian(xi, xj, z)
        assert np.all(np.isfinite(e)) and np.all(np.isfinite(Ji)) and np.all(np.isfinite(Jj))
        assert abs(np.linalg.norm(e[:3]) - angle) <= 1e-9 + 1e-9 * angle
        ni, nj = _num_jac(xi, xj, z)
        assert np.max(np.abs(Ji - ni)) <= 2e-8 * max(1.0, np.max(np.abs(ni)))
        assert np.max(np.abs(Jj - nj)) <= 2e-8 * max(1.0, np.max(np.abs(nj)))


def test_restatement_log_exp_round_trip():
    rng = np.random.default_rng(2)
    for th in (0.0, 1e-12, 1e-6, 0.049, 0.051, 1.5, 3.0, np.pi - 1e-5, np.pi - 1e-9):
        ax = rng.normal(0, 1, 3)
        r = th * ax / np.linalg.norm(ax)
        back = so3_log(so3_exp(r))
        assert np.max(np.abs(back - r)) <= (1e-6 if th > 3.1 else 1e-13)
        assert np.allclose(so3_jr(r) @ so3_jr_inv(r), np.eye(3), atol=1e-9)


@pytest.mark.parametrize("name", ["n4", "n12", "n35loops"])
def test_restatement_lm_reaches_scipys_optimum(name):
    """From the odometry start, pose 0 held: the restatement's LM and scipy's
    least_squares (tight tolerances, the same residual) end at the same cost."""
    from scipy.optimize import least_squares

    xt, edges, meas, info, A, odo = graph(name)
    N = len(xt)
    words = fixed_words(N)

    def fun(p):
        x = np.concatenate([odo[:1], p.reshape(-1, 6)])
        return graph_rj(x, edges, meas, A, jac=False)[1].ravel()

    sol = least_squares(fun, odo[1:].ravel(), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    st = oba.LMState(1e-4)
    x = odo.copy()
    for _ in range(40):
        x, inf = lm_iteration(x, edges, meas, A, st, words)
    c = graph_cost(x, edges, meas, A)
    print(f"{name}: restatement {c:.17g}, scipy {sol.cost:.17g}")
    assert abs(c - sol.cost) <= 1e-12 * sol.cost
    assert np.array_equal(x[0], odo[0])


@pytest.mark.parametrize("loss", ["huber", "soft_l1", "cauchy"])
def test_restatement_robust_gradient_against_central_differences(loss):
    xt, edges, meas, info, A, odo = graph("n12")
    meas = wrong_meas("n12")
    delta = 1.5
    x = odo + np.random.default_rng(3).normal(0, 0.05, odo.shape)
    H, g, cost, _ = dense_system(x, edges, meas, A, None, loss, delta)
    assert abs(cost - graph_cost(x, edges, meas, A, loss, delta)) <= 1e-14 * cost
    num = np.zeros(x.size)
    for c in range(x.size):
        d = np.zeros(x.size)
        d[c] = 1e-6
        num[c] = (graph_cost(x + d.reshape(-1, 6), edges, meas, A, loss, delta)
                  - graph_cost(x - d.reshape(-1, 6), edges, meas, A, loss, delta)) / 2e-6
    assert np.max(np.abs(-g - num)) <= 1e-6 * max(1.0, np.max(np.abs(num)))


@pytest.mark.parametrize("name,which", list(SEEDS))
def test_reference_conditions_hold(name, which):
    """The conditions the GPU comparisons rest on (asserted inside reference_run)."""
    x0, infos, x = reference_run(name, which)
    acc = [i["accepted"] for i in infos]
    print(name, which, "accepted", acc, "rel decrease",
          [f"{abs(i['cost'] - i['cost_new']) / i['cost']:.1e}" for i in infos])
    if which == "a":
        assert sum(acc) >= 1


# ----------------------------------------------------------------------------- CPU: schedule
def _symbolic(t):
    """Run the factor over the lists on a boolean tile matrix; returns the set of
    tiles written.  Every tile touched must lie in the row profile."""
    T, first = t["T"], t["first"]
    touched = set()
    rows, upd = t["rows"], t["upd"].reshape(-1, 2)
    for k in range(T):
        touched.add((k, k))
        for I in rows[t["col_ptr"][k]:t["col_ptr"][k + 1]]:
            assert I > k and first[I] <= k
            touched.add((int(I), k))
        for I, J in upd[t["upd_ptr"][k]:t["upd_ptr"][k + 1]]:
            assert I >= J > k and first[I] <= J, (k, I, J)
            touched.add((int(I), int(J)))
    return touched


@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("full", [False, True])
def test_schedule_properties(name, full):
    from slam355 import posegraph as pg

    N, loops = GRAPHS[name]
    edges = graph(name)[1]
    t = pg.pg_tables(N, edges, full=full)
    T = t["T"]
    assert T == (N + 9) // 10 and t["n_tiles"] == t["rowoff"][-1]
    for i, j in edges:  # the profile contains every edge's tile
        assert t["first"][max(i, j) // 10] <= min(i, j) // 10
    for k in range(T):  # sorted lists, exactly the rows the profile gives
        rk = t["rows"][t["col_ptr"][k]:t["col_ptr"][k + 1]]
        assert list(rk) == [I for I in range(k + 1, T) if t["first"][I] <= k]
        uk = t["upd"].reshape(-1, 2)[t["upd_ptr"][k]:t["upd_ptr"][k + 1]]
        assert [tuple(u) for u in uk] == [(I, J) for a, I in enumerate(rk) for J in rk[:a + 1]]
    touched = _symbolic(t)
    profile = {(I, J) for I in range(T) for J in range(t["first"][I], I + 1)}
    assert touched <= profile
    if full:
        assert len(profile) == T * (T + 1) // 2 == t["n_tiles"]
    # the CSR tables: every (edge, side) once, in edge order; pairs sorted and unique
    ent = t["pose_ent"]
    assert sorted(ent) == list(range(2 * len(edges)))
    for i in range(N):
        own = ent[t["pose_ptr"][i]:t["pose_ptr"][i + 1]]
        assert list(own) == sorted(own) and all(edges.ravel()[q] == i for q in own)
    pij = [tuple(p) for p in t["pair_ij"].reshape(-1, 2)]
    assert pij == sorted(set((min(i, j), max(i, j)) for i, j in edges))
    for q, (lo, hi) in enumerate(pij):
        own = t["pair_ent"][t["pair_ptr"][q]:t["pair_ptr"][q + 1]]
        assert list(own) == sorted(own)
        for en in own:
            i, j = edges[en >> 1]
            assert (min(i, j), max(i, j)) == (lo, hi) and (en & 1) == int(i > j)
    assert sorted(en >> 1 for en in t["pair_ent"]) == list(range(len(edges)))


def test_schedule_known_answers():
    from slam355 import posegraph as pg

    chain = [(i, i + 1) for i in range(34)]
    t = pg.pg_tables(35, chain)  # a pure chain: tile-tridiagonal
    assert list(t["first"]) == [0, 0, 1, 2] and list(t["rowoff"]) == [0, 1, 3, 5, 7]
    assert list(t["rows"]) == [1, 2, 3] and list(t["col_ptr"]) == [0, 1, 2, 3, 3]
    assert t["upd"].reshape(-1, 2).tolist() == [[1, 1], [2, 2], [3, 3]]
    t = pg.pg_tables(35, chain + [(0, 34)])  # + (0, N - 1): the last tile row is full
    assert list(t["first"]) == [0, 0, 1, 0] and list(t["rowoff"]) == [0, 1, 3, 5, 9]
    assert list(t["rows"]) == [1, 3, 2, 3, 3] and list(t["col_ptr"]) == [0, 2, 4, 5, 5]
    assert t["upd"].reshape(-1, 2).tolist() == [[1, 1], [3, 1], [3, 3], [2, 2], [3, 2], [3, 3], [3, 3]]
    s = pg.pg_schedule(35, chain + [(0, 34)])
    assert s.dtype == np.int32 and list(s[:10]) == [pg.PG_MAGIC, 35, 35, 4, 35, 9, 5, 7, 2, 3]
    with pytest.raises(ValueError):
        pg.pg_tables(4, [(0, 0)])
    with pytest.raises(ValueError):
        pg.pg_tables(4, [(0, 4)])


# ----------------------------------------------------------------------------- CPU: C ABI
def _host_problem(N=12, loops=((0, 11), (2, 9))):
    """A descriptor whose host tables are real and whose device pointers are a
    non-null dummy: enough for every refusal, which come before any launch."""
    from slam355 import _lib
    from slam355 import posegraph as pg

    edges = np.array([(i, i + 1) for i in range(N - 1)] + list(loops), np.int32)
    sched = pg.pg_schedule(N, edges)
    s = _lib.PGProblemStruct()
    s.n_poses, s.n_edges, s.loss, s.sched_len, s.loss_scale = N, len(edges), 0, len(sched), 1.0
    dummy = 0x1000
    s.poses[0] = s.poses[1] = dummy
    s.edge_ij = s.meas = s.sqrt_info = s.sched = s.ws = s.state = dummy
    s.edge_ij_host, s.sched_host = edges.ctypes.data, sched.ctypes.data
    s.ws_len = int(_lib.lib.slam_pg_workspace_len(N, len(edges), int(sched[5])))
    return s, edges, sched


def test_descriptor_size_on_both_sides():
    from slam355 import _lib

    assert _lib.lib.slam_pg_problem_size() == ctypes.sizeof(_lib.PGProblemStruct) == 120
    assert _lib.lib.slam_ba_problem_size() == 408 and _lib.lib.slam_abi_version() == 1
    for name in ("slam_pg_problem_size", "slam_pg_workspace_len", "slam_pg_reset", "slam_pg_iterate",
                 "slam_pg_residual", "slam_pg_jacobian"):
        assert name in _lib.SIGNATURES
    assert _lib.lib.slam_pg_workspace_len(0, 1, 1) == -1 and _lib.lib.slam_pg_workspace_len(12, 13, 3) > 0


def _refused(s, needle, code=-1):
    from slam355 import _lib

    calls = {"slam_pg_reset": lambda: _lib.lib.slam_pg_reset(ctypes.byref(s), 1e-4, None),
             "slam_pg_iterate": lambda: _lib.lib.slam_pg_iterate(ctypes.byref(s), 1, None)}
    for name, fn in calls.items():
        rc = fn()
        msg = _lib.lib.slam_last_error()
        assert rc == code and needle in msg, (name, rc, msg)


def test_c_abi_refusals():
    """Each refusal returns -1 (a short workspace: -3) with a message, before any launch."""
    from slam355 import _lib

    lib = _lib.lib
    assert lib.slam_pg_iterate(None, 1, None) == -1 and b"null problem" in lib.slam_last_error()
    for field in ("edge_ij", "edge_ij_host", "meas", "sqrt_info", "sched", "sched_host", "ws", "state"):
        s, edges, sched = _host_problem()
        setattr(s, field, None)
        _refused(s, b"null buffer")
    s, edges, sched = _host_problem()
    s.poses[1] = None
    _refused(s, b"null buffer")
    s, edges, sched = _host_problem()
    s.ws_len -= 1
    _refused(s, b"workspace", code=-3)
    for n, e in ((0, 13), (12, 0), (-1, 13)):
        s, edges, sched = _host_problem()
        s.n_poses, s.n_edges = n, e
        _refused(s, b"N >= 1")
    s, edges, sched = _host_problem()
    edges[3] = (5, 5)
    _refused(s, b"to itself")
    for bad in (12, -1):
        s, edges, sched = _host_problem()
        edges[12, 1] = bad
        _refused(s, b"out of range")
    for loss in (-1, 4):
        s, edges, sched = _host_problem()
        s.loss = loss
        _refused(s, b"loss")
    for scale in (0.0, -1.0, float("nan"), float("inf")):
        s, edges, sched = _host_problem()
        s.loss, s.loss_scale = 1, scale
        _refused(s, b"loss_scale")
    # the residual / Jacobian entry points check the edges and the loss too
    s, edges, sched = _host_problem()
    edges[0] = (0, 99)
    assert lib.slam_pg_residual(ctypes.byref(s), 0x1000, 0x1000, None) == -1
    assert lib.slam_pg_jacobian(ctypes.byref(s), 0x1000, 0x1000, None) == -1
    s, edges, sched = _host_problem()
    assert lib.slam_pg_residual(ctypes.byref(s), None, None, None) == -1 and b"null outputs" in lib.slam_last_error()
    assert lib.slam_pg_jacobian(ctypes.byref(s), 0x1000, None, None) == -1


def test_c_abi_refuses_a_wrong_schedule():
    from slam355 import posegraph as pg

    s0, edges, sched = _host_problem()
    N, E, T, P = (int(v) for v in sched[1:5])
    off_first = pg.PG_HDR
    off_rowoff = off_first + T
    off_pose_ptr = off_rowoff + T + 1
    off_pose_ent = off_pose_ptr + N + 1
    off_pair_ptr = off_pose_ent + 2 * E
    off_pair_ij = off_pair_ptr + P + 1
    off_pair_ent = off_pair_ij + 2 * P
    off_col_ptr = off_pair_ent + E
    off_upd_ptr = off_col_ptr + T + 1
    off_lists = off_upd_ptr + T + 1
    assert off_lists + sched[6] + 2 * sched[7] == len(sched)
    tampers = [(0, 1), (1, N + 1), (3, T + 1), (4, 0), (5, sched[5] + 1), (8, sched[8] + 1),
               (off_first + 1, 1),          # tile row 1 loses its column 0: an edge leaves the profile
               (off_first + 1, 2),          # first[I] > I
               (off_rowoff + 1, 2),
               (off_pose_ptr + 3, 0), (off_pose_ent + 2, 2 * E), (off_pose_ent + 2, -1),
               (off_pair_ptr + 2, 0), (off_pair_ij + 1, N), (off_pair_ij + 2, N - 1),
               (off_pair_ent + 1, int(sched[off_pair_ent + 1]) ^ 1),  # the flip bit
               (off_col_ptr + 1, 0), (off_upd_ptr + 1, 0), (off_lists, 0), (off_lists + int(sched[6]), 0)]
    for idx, val in tampers:
        s, edges, sched = _host_problem()
        sched[idx] = val
        _refused(s, b"schedule")
    s, edges, sched = _host_problem()
    s.sched_len -= 1
    _refused(s, b"schedule")
    # the schedule of another graph of the same sizes: its pairs do not match the edges
    s, edges, sched = _host_problem()
    other = pg.pg_schedule(12, np.array([(i, i + 1) for i in range(11)] + [(0, 10), (2, 9)], np.int32))
    assert len(other) == len(sched)
    sched[:] = other
    _refused(s, b"schedule")


def test_python_argument_checks():
    """PoseGraph's host-side checks that need no device come first."""
    from slam355 import posegraph as pg

    with pytest.raises(ValueError):
        pg._check_edges(3, [(0, 1), (1, 1)])
    with pytest.raises(ValueError):
        pg._check_edges(3, [(0, 3)])
    with pytest.raises(ValueError):
        pg._check_edges(3, np.zeros((0, 2), np.int32))
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.normal(0, 0.5, 3), rng.normal(0, 2, 3)])
    b = np.concatenate([rng.normal(0, 0.5, 3), rng.normal(0, 2, 3)])
    assert np.allclose(pg.relative_pose(a, b), relative_pose(a, b), rtol=0, atol=1e-14)
    G = pg.relative_pose_jacobian(a, b)
    _, Ji, Jj = edge_jacobian(a, b, np.zeros(6))
    assert np.allclose(G, np.concatenate([Ji, Jj], 1), rtol=0, atol=1e-12)
    assert np.allclose(pg.relative_pose(a, a), 0.0, atol=1e-15)


# ----------------------------------------------------------------------------- GPU
def _pg(name, x0, words="default", **kw):
    from slam355 import posegraph as pg

    xt, edges, meas, info, A, odo = graph(name)
    if isinstance(words, str):
        words = fixed_words(len(xt))
    meas = kw.pop("meas", meas)
    return pg.PoseGraph(x0, edges, meas, information=info, fixed=words, **kw)


def _rel(got, ref):
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("loss", ["linear", "soft_l1", "cauchy"])
def test_gpu_residual_and_jacobian_match_restatement(name, loss):
    xt, edges, meas, info, A, odo = graph(name)
    words = fixed_words(len(xt), extra=(2, 0x38))
    x0 = odo + np.random.default_rng(21).normal(0, 0.3, odo.shape) * ~held_mask(words, len(xt))
    assert max_angle(x0, edges, meas) < np.pi - PI_MARGIN
    g = _pg(name, x0, words=words, loss=loss, f_scale=1.5)
    e, rt, Ji, Jj, ct = graph_rj(x0, edges, meas, A, words, loss, 1.5)
    ge, gr = g.residuals(weighted=False), g.residuals()
    gi, gj = g.jacobian()
    print(f"{name} {loss}: e {_rel(ge, e):.1e} r {_rel(gr, rt):.1e} Ji {_rel(gi, Ji):.1e} Jj {_rel(gj, Jj):.1e}")
    assert _rel(ge, e) <= 1e-9 and _rel(gr, rt) <= 1e-9
    assert _rel(gi, Ji) <= 1e-9 and _rel(gj, Jj) <= 1e-9
    held = held_mask(words, len(xt))
    for k, (i, j) in enumerate(edges):  # held columns are exact zeros
        assert np.all(gi[k][:, held[i]] == 0.0) and np.all(gj[k][:, held[j]] == 0.0)
    assert abs(g.state()["COST"] - 0.5 * ct.sum()) <= 1e-9 * 0.5 * ct.sum()


@pytest.mark.gpu
def test_gpu_zero_residual_and_large_angle_edges():
    """Every residual exactly zero (finite Jacobians, not 0/0), and an edge at 3.0 rad."""
    from slam355 import posegraph as pg

    xt, edges, meas, info, A, odo = graph("n12")
    zero = np.stack([pg.relative_pose(xt[i], xt[j]) for i, j in edges])
    g = pg.PoseGraph(xt, edges, zero, information=info)
    e, rt, Ji, Jj, ct = graph_rj(xt, edges, zero, A)
    ge = g.residuals(weighted=False)
    gi, gj = g.jacobian()
    assert np.all(np.isfinite(ge)) and np.all(np.isfinite(gi)) and np.all(np.isfinite(gj))
    assert np.max(np.abs(ge)) <= 1e-14 and np.max(np.abs(e)) <= 1e-14
    assert _rel(gi, Ji) <= 1e-9 and _rel(gj, Jj) <= 1e-9
    # one measurement exactly the identity between two equal poses: e = 0 bit for bit
    x2 = xt[:2].copy()
    x2[1] = x2[0]
    g2 = pg.PoseGraph(x2, [(0, 1)], np.zeros((1, 6)))
    assert np.all(g2.residuals(weighted=False) == 0.0)
    j2 = g2.jacobian()
    assert np.all(np.isfinite(j2[0])) and np.all(np.isfinite(j2[1]))
    _, ri, rj = edge_jacobian(x2[0], x2[1], np.zeros(6))
    assert _rel(j2[0][0], ri) <= 1e-9 and _rel(j2[1][0], rj) <= 1e-9
    # 3.0 rad
    big = zero.copy()
    off = np.concatenate([3.0 * np.array([0.6, -0.64, 0.48]), [0.2, 0.1, -0.3]])
    # Z = T_rel T_off^-1, so that E = Z^-1 T_rel = T_off
    big[3] = relative_pose(compose(off, relative_pose(zero[3], np.zeros(6))), np.zeros(6))
    g3 = pg.PoseGraph(xt, edges, big, information=info)
    e, rt, Ji, Jj, ct = graph_rj(xt, edges, big, A)
    assert abs(np.linalg.norm(e[3, :3]) - 3.0) <= 1e-9
    gi, gj = g3.jacobian()
    assert _rel(g3.residuals(weighted=False), e) <= 1e-9 and _rel(g3.residuals(), rt) <= 1e-9
    assert _rel(gi, Ji) <= 1e-9 and _rel(gj, Jj) <= 1e-9


def _compare_iterates(g, infos, tag):
    for n, inf in enumerate(infos):
        g.iterate(1)
        s = g.state()
        x = g.poses()
        print(f"{tag} it {n}: acc {int(s['ACCEPTED'])}/{int(inf['accepted'])} cost_new {s['COST_NEW']:.12g} "
              f"ref {inf['cost_new']:.12g} lam {s['LAMBDA']:.6g} ref {inf['lam_out']:.6g} "
              f"dx {np.max(np.abs(x - inf['x_out'])):.2e}")
        assert s["CHOL_FAIL"] == 0.0
        assert bool(s["ACCEPTED"]) == inf["accepted"]
        assert abs(s["COST_NEW"] - inf["cost_new"]) <= 1e-8 * inf["cost_new"]
        assert abs(s["LAMBDA"] - inf["lam_out"]) <= 1e-6 * inf["lam_out"]
        assert np.allclose(x, inf["x_out"], rtol=1e-6, atol=1e-9)
        assert int(s["NACCEPT"]) == sum(i["accepted"] for i in infos[:n + 1]) and int(s["ITERS"]) == n + 1


@pytest.mark.gpu
@pytest.mark.parametrize("name,which", list(SEEDS))
def test_gpu_lm_iterates_match_restatement(name, which):
    x0, infos, xf = reference_run(name, which)
    g = _pg(name, x0, lam0=LAM0)
    _compare_iterates(g, infos, f"{name}/{which}")
    assert np.array_equal(g.poses()[0], x0[0])


@pytest.mark.gpu
def test_gpu_held_parameters():
    """Pose 0 whole and pose 4's translation: bits unchanged in both buffers after
    6 iterations; nothing held: the damping carries the gauge."""
    xt, edges, meas, info, A, odo = graph("n12")
    x0 = odo + np.random.default_rng(4).normal(0, 0.05, odo.shape)
    words = fixed_words(12, extra=(4, 0x38))
    g = _pg("n12", x0, words=words)
    g.iterate(6)
    s = g.state()
    assert s["CHOL_FAIL"] == 0.0 and s["NACCEPT"] >= 1
    for buf in ("x0", "x1"):
        x = g.t[buf].cpu().numpy().reshape(12, 6)
        assert np.array_equal(x[0].view(np.uint64), x0[0].view(np.uint64))
        assert np.array_equal(x[4, 3:].view(np.uint64), x0[4, 3:].view(np.uint64))
    assert not np.array_equal(g.poses()[4, :3], x0[4, :3])
    free = _pg("n12", x0, words=None)
    free.iterate(6)
    s = free.state()
    assert s["CHOL_FAIL"] == 0.0 and s["NACCEPT"] >= 1 and np.all(np.isfinite(free.poses()))


@pytest.mark.gpu
@pytest.mark.parametrize("loss", ["huber", "cauchy"])
def test_gpu_robust_iterates_match_restatement(loss):
    x0, infos, xf = reference_run("n12", "r", loss, ROBUST_DELTA, True)
    g = _pg("n12", x0, lam0=LAM0, loss=loss, f_scale=ROBUST_DELTA, meas=wrong_meas("n12"))
    _compare_iterates(g, infos, f"n12/{loss}")


@pytest.mark.gpu
def test_gpu_all_inlier_huber_equals_linear_bitwise():
    xt, edges, meas, info, A, odo = graph("n12")
    x0 = odo + np.random.default_rng(4).normal(0, 0.02, odo.shape) * ~held_mask(fixed_words(12), 12)
    r = graph_rj(x0, edges, meas, A)[1]
    delta = 10.0 * float(np.sqrt(np.max(np.sum(r * r, 1))))
    lin, hub = _pg("n12", x0), _pg("n12", x0, loss="huber", f_scale=delta)
    lin.iterate(4)
    hub.iterate(4)
    assert lin.state()["NACCEPT"] >= 1
    assert np.array_equal(lin.poses().view(np.uint64), hub.poses().view(np.uint64))
    assert np.array_equal(lin.t["state"].cpu().numpy().view(np.uint64), hub.t["state"].cpu().numpy().view(np.uint64))


@pytest.mark.gpu
def test_gpu_cauchy_beats_linear_with_wrong_loop_edges():
    xt, edges, meas, info, A, odo = graph("n12")
    err = {}
    for loss in ("linear", "cauchy"):
        g = _pg("n12", odo.copy(), loss=loss, f_scale=ROBUST_DELTA, meas=wrong_meas("n12"))
        g.iterate(30)
        assert g.state()["CHOL_FAIL"] == 0.0
        err[loss] = float(np.mean(np.linalg.norm(g.poses()[:, 3:] - xt[:, 3:], axis=1)))
    print(f"mean translation error: linear {err['linear']:.4f} m, cauchy {err['cauchy']:.4f} m")
    assert err["cauchy"] < err["linear"]


@pytest.mark.gpu
def test_gpu_determinism():
    x0 = start_of("n35loops", "a")
    a, b, c = (_pg("n35loops", x0, lam0=LAM0) for _ in range(3))
    a.iterate(3)
    a.iterate(3)
    b.iterate(6)
    c.iterate(6)
    bits = lambda g: (g.poses().view(np.uint64), g.t["state"].cpu().numpy().view(np.uint64))  # noqa: E731
    for u, v in ((a, b), (b, c)):
        assert np.array_equal(bits(u)[0], bits(v)[0]) and np.array_equal(bits(u)[1], bits(v)[1])
    assert b.state()["NACCEPT"] >= 1


@pytest.mark.gpu
def test_gpu_zero_residual_graph_stays_put():
    from slam355 import posegraph as pg

    xt, edges, meas, info, A, odo = graph("n12")
    x2 = np.tile(xt[3], (12, 1))  # equal poses, identity measurements: every residual is exactly 0
    g = pg.PoseGraph(x2, edges, np.zeros((len(edges), 6)), information=info, fixed=fixed_words(12))
    g.iterate(3)
    s = g.t["state"].cpu().numpy()
    assert np.all(np.isfinite(s)) and g.state()["COST"] == 0.0 and g.state()["CHOL_FAIL"] == 0.0
    for buf in ("x0", "x1"):
        assert np.array_equal(g.t[buf].cpu().numpy().reshape(12, 6).view(np.uint64), x2.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n35loops", "n35chain", "n45loop"])
def test_gpu_skyline_equals_full_profile(name):
    """The profile forced full (first[I] = 0): the same accept sequence, poses
    within the bars.  The loop graph's own profile is already the full lower
    triangle of its four tile rows; the chain stores 7 of 10 tiles and has no
    fill; n45loop stores 10 of 15 with fill inside the profile."""
    x0, infos, xf = reference_run(name, "b")
    sky, full = _pg(name, x0, lam0=LAM0), _pg(name, x0, lam0=LAM0, _full_profile=True)
    T = (GRAPHS[name][0] + 9) // 10
    assert full.n_tiles == T * (T + 1) // 2 and sky.n_tiles == {"n35loops": 10, "n35chain": 7, "n45loop": 10}[name]
    for n in range(len(infos)):
        sky.iterate(1)
        full.iterate(1)
        assert sky.state()["ACCEPTED"] == full.state()["ACCEPTED"] == float(infos[n]["accepted"])
        assert full.state()["CHOL_FAIL"] == 0.0
    assert np.allclose(sky.poses(), full.poses(), rtol=1e-6, atol=1e-9)
    assert np.allclose(full.poses(), xf, rtol=1e-6, atol=1e-9)


@pytest.mark.gpu
def test_gpu_factor_that_is_not_positive_definite_takes_the_zero_step():
    """Square-root information of 1e200 overflows H to inf: the first pivot is
    not finite, so CHOL_FAIL = 1, the step is the zero step and is rejected,
    lambda grows by nu, and the next iteration does the same (the flag is
    cleared and raised again).  Column 0 of this graph has three panel-row
    workgroups beside the diagonal one."""
    from slam355 import posegraph as pg

    xt, edges, meas, info, A, odo = graph("n35loops")
    g = pg.PoseGraph(odo, edges, meas, sqrt_information=1e200 * A, fixed=fixed_words(35), lam0=1e-4)
    for n in range(2):
        g.iterate(1)
        s = g.state()
        assert s["CHOL_FAIL"] == 1.0 and s["ACCEPTED"] == 0.0 and s["NACCEPT"] == 0.0 and s["ITERS"] == n + 1
        assert s["RHO"] == -1.0 and s["CUR"] == 0.0
        assert s["LAMBDA"] == 1e-4 * (2.0 if n == 0 else 8.0) and s["NU"] == (4.0 if n == 0 else 8.0)
        for buf in ("x0", "x1"):
            assert np.array_equal(g.t[buf].cpu().numpy().reshape(35, 6).view(np.uint64), odo.view(np.uint64))


@pytest.mark.gpu
def test_gpu_solve_converges_to_scipys_optimum():
    from scipy.optimize import least_squares

    xt, edges, meas, info, A, odo = graph("n12")
    g = _pg("n12", odo.copy())
    st = g.solve(max_iter=60)

    def fun(p):
        return graph_rj(np.concatenate([odo[:1], p.reshape(-1, 6)]), edges, meas, A, jac=False)[1].ravel()

    sol = least_squares(fun, odo[1:].ravel(), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    assert abs(st["COST"] - sol.cost) <= 1e-9 * sol.cost


@pytest.mark.gpu
def test_gpu_edges_from_ba():
    """Information of (2,3) and (2,9) from the device covariance against the same
    propagation from np.linalg.inv of the full free H (test_ba_cov's reference,
    measure and run-time bar); the graph built from the edges has zero residuals."""
    import test_ba_cov as tc
    from slam355 import ba
    from slam355 import posegraph as pg
    from slam355.synthetic import perturb

    cams, pts, ci, pi, qs = tc.problem("10x300")
    C = len(cams)
    fx = tc.gauge(C, False)
    prob = ba.BAProblem(*perturb(np.random.default_rng(5), cams, pts), ci, pi, qs, fixed=fx)
    prob.iterate(3)
    lc, lp = prob.params()
    full, spread, cond = tc.sigma_reference(lc, lp, ci, pi, qs, fx)
    assert spread <= tc.SPREAD_MAX
    pairs = [(2, 3), (2, 9)]
    edges, meas, info = pg.edges_from_ba(prob, pairs)
    worst = 0.0
    for q, (a, b) in enumerate(pairs):
        S = np.block([[full[9 * a:9 * a + 6, 9 * a:9 * a + 6], full[9 * a:9 * a + 6, 9 * b:9 * b + 6]],
                      [full[9 * b:9 * b + 6, 9 * a:9 * a + 6], full[9 * b:9 * b + 6, 9 * b:9 * b + 6]]])
        _, Ji, Jj = edge_jacobian(lc[a, :6], lc[b, :6], np.zeros(6))
        G = np.concatenate([Ji, Jj], 1)
        ref = np.linalg.inv(G @ S @ G.T)
        d = np.sqrt(np.diag(ref))
        worst = max(worst, float(np.max(np.abs(info[q] - ref) / np.outer(d, d))))
        assert np.allclose(meas[q], relative_pose(lc[a, :6], lc[b, :6]), rtol=0, atol=1e-13)
    print(f"edges_from_ba: deviation {worst:.2e}, spread {spread:.2e}, bar {tc.MARGIN * spread:.2e}")
    assert worst <= tc.MARGIN * spread
    g = pg.PoseGraph(lc[:, :6], edges, meas, information=info)
    assert np.max(np.abs(g.residuals(weighted=False))) <= 1e-13
    with pytest.raises(np.linalg.LinAlgError):
        pg.edges_from_ba(prob, [(0, 1)])  # two held cameras: no covariance to invert
