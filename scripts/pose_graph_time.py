"""Time per LM iteration of posegraph.PoseGraph (profiles/pose_graph/).

    python scripts/pose_graph_time.py loop500|back500|big5000 [full|cov]

`cov` (profiles/pg_cov/): HIP events around one covariance() call
for the last pose's block and one for 8 poses spread over the trajectory, median
of 5 after a warm-up, beside the launch count and the host yardstick of the same
request (scipy.sparse.linalg.splu of H0 plus the solves for the poses' columns).

Otherwise: HIP events around iterate(1), median of 5 after one warm-up; the launch count
per iteration and the tiles of the row profile against T (T + 1) / 2.  `full`
forces the profile full (first[I] = 0): the same kernels without the skyline
(not at big5000: 125 250 tiles).  Yardsticks that are not the code under test:
one LM step's linear solve of the same damped system on the host
(scipy.sparse.linalg.spsolve on the CSC matrix; dense NumPy without scipy).
One JSON line.

Shapes: loop500 500 poses, chain + (0, 499); back500 500 poses, chain + 11
loop edges reaching back 250; big5000 5000 poses, chain + 50 loop edges.
Pose 0 is held whole; the start is the odometry.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "slam-1_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from slam355 import posegraph as pg  # noqa: E402


def make(name):
    rng = np.random.default_rng(7)
    if name == "loop500":
        N, loops = 500, [(0, 499)]
    elif name == "back500":
        N, loops = 500, [(i - 250, i) for i in range(260, 500, 22)][:11]
    elif name == "big5000":
        N = 5000
        loops = [(int(j - rng.integers(50, 400)), int(j)) for j in np.linspace(450, 4999, 50).astype(int)]
    else:
        raise SystemExit(f"unknown shape {name}")
    i = np.arange(N, dtype=np.float64)
    turns = max(1.0, N / 500.0)
    x = np.zeros((N, 6))
    x[:, 0] = 0.15 * np.sin(0.35 * i)
    x[:, 1] = 0.5 * np.sin(2.0 * np.pi * turns * i / N)
    x[:, 2] = 0.1 * np.cos(0.2 * i)
    x[:, 3] = 40.0 * np.cos(2.0 * np.pi * turns * i / N)
    x[:, 4] = 40.0 * np.sin(2.0 * np.pi * turns * i / N)
    x[:, 5] = 0.3 * np.sin(0.5 * i)
    edges = np.array([(k, k + 1) for k in range(N - 1)] + loops, np.int32)
    meas = np.stack([pg.relative_pose(x[a], x[b]) for a, b in edges]) + rng.normal(0, 0.01, (len(edges), 6))
    odo = np.zeros_like(x)
    odo[0] = x[0]
    for k in range(N - 1):  # x_{k+1} = x_k o z_k
        Rk = pg._so3_exp(odo[k, :3])
        odo[k + 1, :3] = pg._so3_log(Rk @ pg._so3_exp(meas[k, :3]))
        odo[k + 1, 3:] = odo[k, 3:] + Rk @ meas[k, 3:]
    fixed = np.zeros(N, np.uint32)
    fixed[0] = pg.FIXED_POSE
    return odo, edges, meas, fixed


def timed(fn, reps=5):
    fn()  # warm-up
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [round(m, 3) for m in ms]


def host_solve_ms(g, lam=1e-4):
    """The damped system of one LM step from the device Jacobians, solved on the
    host: median of 5 solves after a warm-up, the system formed beforehand."""
    Ji, Jj = g.jacobian()
    r = g.residuals().ravel()
    N, E = g.N, g.E
    rows = (6 * np.arange(E)[:, None, None] + np.arange(6)[None, :, None]) + np.zeros((1, 1, 6), np.int64)
    ci = 6 * g.edges[:, 0].astype(np.int64)[:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 6, 1), np.int64)
    cj = 6 * g.edges[:, 1].astype(np.int64)[:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 6, 1), np.int64)
    try:
        import scipy.sparse as sp
        from scipy.sparse.linalg import spsolve

        J = sp.csr_matrix((np.concatenate([Ji.ravel(), Jj.ravel()]),
                           (np.concatenate([rows.ravel(), rows.ravel()]), np.concatenate([ci.ravel(), cj.ravel()]))),
                          shape=(6 * E, 6 * N))
        H = (J.T @ J).tocsc()
        D = np.clip(H.diagonal(), 1e-6, 1e32)
        Hd, rhs = (H + sp.diags(lam * D, format="csc")).tocsc(), -(J.T @ r)
        solve, how = (lambda: spsolve(Hd, rhs)), "scipy.sparse.linalg.spsolve"
    except ImportError:
        J = np.zeros((6 * E, 6 * N))
        J[rows.ravel(), ci.ravel()] = Ji.ravel()
        J[rows.ravel(), cj.ravel()] += Jj.ravel()
        H = J.T @ J
        Hd, rhs = H + np.diag(lam * np.clip(np.diag(H), 1e-6, 1e32)), -(J.T @ r)
        solve, how = (lambda: np.linalg.solve(Hd, rhs)), "numpy.linalg.solve (dense)"
    solve()  # warm-up
    ts = []
    for _ in range(5):  # the solve alone: H, D and g are formed outside the timed region
        t0 = time.perf_counter()
        d = solve()
        ts.append(1e3 * (time.perf_counter() - t0))
    ms = float(np.median(ts))
    assert np.all(np.isfinite(d))
    return ms, how


def host_cov_ms(g, poses):
    """The host yardstick of a covariance request: scipy.sparse.linalg.splu of
    the free H0 (undamped, from the device Jacobians, formed beforehand) plus
    the solves for the 6 columns of every requested pose; median of 5 after a
    warm-up.  None without scipy."""
    try:
        import scipy.sparse as sp
        from scipy.sparse.linalg import splu
    except ImportError:
        return None, None
    Ji, Jj = g.jacobian()
    N, E = g.N, g.E
    rows = (6 * np.arange(E)[:, None, None] + np.arange(6)[None, :, None]) + np.zeros((1, 1, 6), np.int64)
    ci = 6 * g.edges[:, 0].astype(np.int64)[:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 6, 1), np.int64)
    cj = 6 * g.edges[:, 1].astype(np.int64)[:, None, None] + np.arange(6)[None, None, :] + np.zeros((1, 6, 1), np.int64)
    J = sp.csr_matrix((np.concatenate([Ji.ravel(), Jj.ravel()]),
                       (np.concatenate([rows.ravel(), rows.ravel()]), np.concatenate([ci.ravel(), cj.ravel()]))),
                      shape=(6 * E, 6 * N))
    H = (J.T @ J).tocsc()[6:, 6:].tocsc()  # pose 0 is held whole
    rhs = np.zeros((6 * N - 6, 6 * len(poses)))
    for q, a in enumerate(poses):
        rhs[6 * (a - 1):6 * a, 6 * q:6 * q + 6] = np.eye(6)

    def solve():
        return splu(H).solve(rhs)

    solve()
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        x = solve()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), x


def cov_main(name):
    """`cov`: one covariance() call for the last pose's block and one for 8 poses
    spread over the trajectory (8 distinct tile columns), DESIGN.md 4e."""
    odo, edges, meas, fixed = make(name)
    g = pg.PoseGraph(odo, edges, meas, fixed=fixed)
    t = pg.pg_tables(g.N, edges)
    T = t["T"]
    factor = 3 + T + int(np.count_nonzero(np.diff(t["upd_ptr"])))
    out = dict(shape=name, mode="cov", poses=g.N, edges=g.E, T=T, tiles=int(t["n_tiles"]), factor_launches=factor)
    for tag, poses in (("last", [g.N - 1]), ("spread8", [int(v) for v in np.linspace(g.N // 16, g.N - 1, 8)])):
        plan = pg.pg_cov_plan(g.N, [(a, a) for a in poses])
        launches = factor + 2 + (T - int(plan["cols"].min())) + (T - int(plan["low"].min())) + 1
        ms, all_ms = timed(lambda: g.covariance(poses=poses, device=True))
        cov = g.covariance(poses=poses)
        hs, x = host_cov_ms(g, poses)
        out[tag] = dict(poses=poses, cols=int(len(plan["cols"])), launches=launches, ms=round(ms, 3), ms_all=all_ms,
                        us_per_launch=round(1e3 * ms / launches, 2), status=g.cov_status())
        if hs is not None:
            dev = 0.0
            for q, a in enumerate(poses):  # the device blocks against the host solve, the tests' measure
                ref = x[6 * (a - 1):6 * a, 6 * q:6 * q + 6]
                d = np.sqrt(np.diag(ref))
                dev = max(dev, float(np.max(np.abs(cov[q] - ref) / np.outer(d, d))))
            out[tag].update(host_splu_ms=round(hs, 3), deviation_from_host=dev)
    print(json.dumps(out))


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "loop500"
    if len(sys.argv) > 2 and sys.argv[2] == "cov":
        return cov_main(name)
    full = len(sys.argv) > 2 and sys.argv[2] == "full"
    odo, edges, meas, fixed = make(name)
    g = pg.PoseGraph(odo, edges, meas, fixed=fixed, _full_profile=full)
    t = pg.pg_tables(g.N, edges, full=full)
    T = t["T"]
    launches = 3 + T + int(np.count_nonzero(np.diff(t["upd_ptr"]))) + T + 2
    ms, all_ms = timed(lambda: g.iterate(1))
    st = g.state()
    out = dict(shape=name, full=full, poses=g.N, edges=g.E, T=T, tiles=int(t["n_tiles"]), tiles_dense=T * (T + 1) // 2,
               update_pairs=int(len(t["upd"]) // 2), launches_per_iter=launches, ms_per_iter=round(ms, 3), ms_all=all_ms,
               cost=st["COST"], naccept=st["NACCEPT"], chol_fail=st["CHOL_FAIL"])
    if not full:
        hs, how = host_solve_ms(g)
        out.update(host_solve_ms=round(hs, 3), host_solver=how)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
