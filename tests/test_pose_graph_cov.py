"""Pose and relative-pose covariance of the SE(3) pose graph and the gate of
loop-closure candidates (slam_pg_covariance / slam_pg_gate, PoseGraph.covariance
/ relative_covariance / gate, pg_cov_plan).

Semantics (include/slam355.h): Sigma = H0^-1 on the free parameters, H0 = J~^T
J~ at the live poses with zero damping, J~ the robust-weighted, A-weighted
Jacobian without the held columns; rows and columns of held parameters +0.0;
the caller holds one pose.  The gate of a candidate (i, j, z, A): e, J_i, J_j of
that edge with nothing held and no weight, P = [J_i J_j] [S_ii S_ij; S_ji S_jj]
[J_i J_j]^T, R = (A^T A)^-1, d2 = e^T (P + R)^-1 e.

Reference: the NumPy restatement of tests/test_pose_graph.py (imported):
np.linalg.inv of the free rows and columns of dense_system's H.

Measure of a block: max |dSigma_pq| / sqrt(Sigma_pp Sigma_qq).  Bar: 100 x the
reference's own spread on that graph and point, the largest deviation in the
same measure (over the whole free matrix) among np.linalg.inv, a Cholesky solve
and the QR of J~ -- the margin test_gpu_edges_from_ba gives a GPU covariance
over a two-route spread.  The gate: e at 1e-9 relative, P at the block bar
scaled by P's own diagonal, d2 relative at cond(S_k) x that bar, accept equal.

Graphs: those of test_pose_graph.py (n4: T = 1, both sweeps degenerate; n12:
two poses in the last tile, padding rows; n35chain; n35loops; n45loop: a
partial profile with fill, requests outside the profile) and n95, the same
recipe with loops (5, 90) and (33, 61): T = 10, several columns with different
start tiles and depths in one call.  Points: the odometry start and the point
the restatement's LM converges to.  Pose 0 held whole.
"""
import ctypes
import functools

import numpy as np
import pytest

import test_pose_graph as tp
from oracle import ba as oba

MARGIN = 100.0
RANK_TOL = 1e-8
CHI2 = 16.811893829770927
N95 = (95, [(5, 90), (33, 61)])
NAMES = ["n4", "n12", "n35chain", "n35loops", "n45loop", "n95"]
# requests outside the row profile (n45loop: first = 0 0 1 1 3)
OUTSIDE = {"n45loop": [(2, 44), (40, 7)], "n95": [(3, 94), (88, 12)]}
GATE_SCALE = 50.0  # A x 50: information x 2500, sigma about the 0.01 measurement noise
CANDS = {"n12": [(1, 8), (10, 3), (0, 6)], "n45loop": [(2, 44), (40, 7), (12, 38), (44, 43)]}
WRONG = np.array([0.3, 0.3, 0.25, 1.2, 1.2, 1.0])
GATE_SEED = {"n12": 0, "n45loop": 0}  # checked on the CPU: test_gate_conditions_hold_on_the_reference


# ----------------------------------------------------------------------------- inputs and reference
@functools.lru_cache(maxsize=None)
def graph(name):
    """tp.graph, and n95 by the same recipe."""
    if name != "n95":
        return tp.graph(name)
    N, loops = N95
    rng = np.random.default_rng(11)
    xt = tp.truth(N)
    edges = np.array([(i, i + 1) for i in range(N - 1)] + loops, np.int32)
    meas = np.stack([tp.relative_pose(xt[i], xt[j]) for i, j in edges])
    meas = meas + rng.normal(0, 0.01, meas.shape)
    M = rng.normal(0, 1.0, (len(edges), 6, 6))
    info = 4.0 * np.eye(6) + 0.5 * M @ M.transpose(0, 2, 1)
    A = np.stack([np.linalg.cholesky(m).T for m in info])
    odo = np.zeros((N, 6))
    odo[0] = xt[0]
    for i in range(N - 1):
        odo[i + 1] = tp.compose(odo[i], meas[i])
    for a in (xt, edges, meas, info, A, odo):
        a.setflags(write=False)
    return xt, edges, meas, info, A, odo


def loss_delta(loss):
    return tp.ROBUST_DELTA if loss != "linear" else 1.0


@functools.lru_cache(maxsize=None)
def point(name, which, loss="linear", scale=1.0):
    """The odometry start ("odo") or the point the restatement's LM reaches
    from it in 25 iterations ("conv"), pose 0 held; never written."""
    xt, edges, meas, info, A, odo = graph(name)
    if which == "odo":
        return odo
    words = tp.fixed_words(len(xt))
    st = oba.LMState(1e-4)
    x = odo.copy()
    for _ in range(25):
        x, _ = tp.lm_iteration(x, edges, meas, scale * A, st, words, loss, loss_delta(loss))
    x.setflags(write=False)
    return x


def measure(S, ref, diag=None):
    d = np.sqrt(np.diag(ref) if diag is None else diag)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.abs(S - ref) / np.outer(d, d)
    return float(np.nanmax(np.where(np.outer(d, d) > 0, q, 0.0)))


def sigma_reference(x, edges, meas, A, words, loss="linear", delta=1.0):
    """(Sigma [6N, 6N] with zero rows and columns on held parameters, spread):
    np.linalg.inv of the free H; the spread among it, a Cholesky solve and the
    QR of the free columns of J~."""
    H, g, cost, Jd = tp.dense_system(x, edges, meas, A, words, loss, delta)
    free = ~tp.held_mask(words, len(x)).ravel()
    Hf = H[np.ix_(free, free)]
    s_inv = np.linalg.inv(Hf)
    Lc = np.linalg.cholesky(Hf)
    Li = np.linalg.solve(Lc, np.eye(len(Hf)))
    s_chol = Li.T @ Li
    R = np.linalg.qr(Jd[:, free], mode="r")
    Ri = np.linalg.solve(R, np.eye(len(Hf)))
    s_qr = Ri @ Ri.T
    spread = max(measure(s_chol, s_inv), measure(s_qr, s_inv), measure(s_qr, s_chol, np.diag(s_inv)))
    full = np.zeros_like(H)
    full[np.ix_(free, free)] = s_inv
    return full, spread


def block(S, a, b):
    return S[6 * a:6 * a + 6, 6 * b:6 * b + 6]


def block_dev(got, S, a, b):
    d = np.sqrt(np.maximum(np.diag(S), 0.0))
    da, db = d[6 * a:6 * a + 6], d[6 * b:6 * b + 6]
    den = np.outer(da, db)
    err = np.abs(got - block(S, a, b))
    assert np.all(got[den == 0] == 0.0)
    return float(np.max(np.where(den > 0, err / np.where(den > 0, den, 1.0), 0.0)))


def request(name):
    """All marginals (poses=None form is tested apart), every edge's pair, the
    pairs outside the profile, one pair in both orders, one repeated entry."""
    N = len(graph(name)[0])
    edges = graph(name)[1]
    pairs = [tuple(int(v) for v in e) for e in edges] + OUTSIDE.get(name, [(0, N - 1), (N - 1, 1)])
    pairs += [(1, N - 2), (N - 2, 1), pairs[0]]
    return np.array([(i, i) for i in range(N)] + pairs, np.int32)


def pivot_ratio(H):
    """min over the pivots met by the unpivoted Cholesky of d_j / H_jj, up to
    and with the first one that is not positive."""
    A = H.copy()
    worst = np.inf
    for j in range(len(A)):
        worst = min(worst, A[j, j] / H[j, j])
        if not A[j, j] > 0.0:
            break
        A[j + 1:, j] /= np.sqrt(A[j, j])
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    return worst


def gate_inputs(name):
    """(x at the converged point of the graph with information x 2500, cands,
    candidate sqrt-information, good measurements, wrong measurements)."""
    xt, edges, meas, info, A, odo = graph(name)
    x = point(name, "conv", "linear", GATE_SCALE)
    cands = np.array(CANDS[name], np.int32)
    rng = np.random.default_rng(GATE_SEED[name])
    M = rng.normal(0, 1.0, (len(cands), 6, 6))
    cinfo = GATE_SCALE ** 2 * (4.0 * np.eye(6) + 0.5 * M @ M.transpose(0, 2, 1))
    cA = np.stack([np.linalg.cholesky(m).T for m in cinfo])
    true = np.stack([tp.relative_pose(xt[i], xt[j]) for i, j in cands])
    good = true + np.stack([np.linalg.solve(cA[k], rng.normal(0, 1.0, 6)) for k in range(len(cands))])  # N(0, R_k)
    return x, cands, cA, good, true + WRONG


def gate_reference(x, S, cands, zs, cA):
    """(e, P, d2, cond S_k) of the restatement."""
    e, P, d2, cond = [], [], [], []
    for k, (i, j) in enumerate(cands):
        ek, Ji, Jj = tp.edge_jacobian(x[i], x[j], zs[k])
        G = np.concatenate([Ji, Jj], 1)
        Sb = np.block([[block(S, i, i), block(S, i, j)], [block(S, j, i), block(S, j, j)]])
        Pk = G @ Sb @ G.T
        Sk = Pk + (np.linalg.inv(cA[k].T @ cA[k]) if cA is not None else 0.0)
        e.append(ek)
        P.append(Pk)
        d2.append(float(ek @ np.linalg.solve(Sk, ek)))
        cond.append(float(np.linalg.cond(Sk)))
    return np.array(e), np.array(P), np.array(d2), np.array(cond)


# ----------------------------------------------------------------------------- CPU
def test_cov_plan_known_answers():
    from slam355 import posegraph as pg

    p = pg.pg_cov_plan(45, [(2, 44), (44, 2)])  # a pair in both orders: one canonical request
    assert p["requests"].tolist() == [[2, 44], [2, 44]] and p["cols"].tolist() == [4] and p["low"].tolist() == [0]
    p = pg.pg_cov_plan(45, [(2, 44), (40, 7)])
    assert p["cols"].tolist() == [4] and p["low"].tolist() == [0]
    p = pg.pg_cov_plan(45, [(12, 38)])
    assert p["cols"].tolist() == [3] and p["low"].tolist() == [1]
    p = pg.pg_cov_plan(45, [(12, 38), (12, 38), (38, 12), (44, 43), (9, 9), (44, 21)])  # repeated entries
    assert p["requests"].tolist() == [[12, 38], [12, 38], [12, 38], [43, 44], [9, 9], [21, 44]]
    assert p["cols"].tolist() == [0, 3, 4] and p["low"].tolist() == [0, 1, 2]
    p = pg.pg_cov_plan(45, [(i, i) for i in range(45)])  # every marginal: every column, its own row
    assert p["cols"].tolist() == [0, 1, 2, 3, 4] and p["low"].tolist() == [0, 1, 2, 3, 4]
    p = pg.pg_cov_plan(45, [(12, 38)], gate=True)  # a candidate needs both poses' own blocks too
    assert p["cols"].tolist() == [1, 3] and p["low"].tolist() == [1, 1]
    assert p["requests"].dtype == p["cols"].dtype == p["low"].dtype == np.int32
    for bad in ([(0, 45)], [(-1, 2)], [], [(0.5, 1.0)], [1, 2], [(True, False)]):
        with pytest.raises(ValueError):
            pg.pg_cov_plan(45, bad)


def _cov_call(s, pairs, n=None, rank_tol=RANK_TOL, d_pairs=0x1000, host="own", d_cov=0x1000, d_ws=0x1000,
              ws_len=None, d_status=0x1000):
    from slam355 import _lib

    pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    if ws_len is None:
        ws_len = 1 << 40
    hp = pr.ctypes.data if host == "own" else host
    rc = _lib.lib.slam_pg_covariance(ctypes.byref(s), d_pairs, hp, len(pr) if n is None else n, rank_tol, d_cov,
                                     d_ws, ws_len, d_status, None)
    return rc, _lib.lib.slam_last_error()


def _gate_call(s, cands, n=None, rank_tol=RANK_TOL, d_cand=0x1000, host="own", d_meas=0x1000, d_A=None,
               outs=(0x1000, 0x1000, 0x1000), d_ws=0x1000, ws_len=None, d_status=0x1000):
    from slam355 import _lib

    pr = np.ascontiguousarray(cands, np.int32).reshape(-1, 2)
    if ws_len is None:
        ws_len = 1 << 40
    hp = pr.ctypes.data if host == "own" else host
    rc = _lib.lib.slam_pg_gate(ctypes.byref(s), d_cand, hp, d_meas, d_A, len(pr) if n is None else n, rank_tol,
                               outs[0], outs[1], outs[2], d_ws, ws_len, d_status, None)
    return rc, _lib.lib.slam_last_error()


def test_c_abi_cov_refusals():
    """Every refusal of slam_pg_covariance / slam_pg_gate comes before any
    launch: -1 (a short workspace: -3) with a message, on a descriptor whose
    device pointers are dummies."""
    from slam355 import _lib

    lib = _lib.lib
    for name in ("slam_pg_cov_workspace_len", "slam_pg_covariance", "slam_pg_gate"):
        assert name in _lib.SIGNATURES
    assert lib.slam_abi_version() == 1 and lib.slam_pg_problem_size() == 120
    # the workspace length: T tiles per column after the tables
    assert lib.slam_pg_cov_workspace_len(12, 1) > 2 * 4096 and lib.slam_pg_cov_workspace_len(12, 2) > 4 * 4096
    assert (lib.slam_pg_cov_workspace_len(12, 2) - lib.slam_pg_cov_workspace_len(12, 1)) == 2 * 4096
    for n, c in ((0, 1), (12, 0), (12, 3), (-5, 1), (2 ** 31 - 1, 1), (-2 ** 31, 1), ((1 << 24) + 1, 1)):
        assert lib.slam_pg_cov_workspace_len(n, c) == -1 and b"slam_pg_cov_workspace_len" in lib.slam_last_error()
    s, edges, sched = tp._host_problem()
    ok = [(0, 0), (3, 11)]
    calls = (("slam_pg_covariance", _cov_call), ("slam_pg_gate", _gate_call))
    for who, call in calls:
        lst = ok if call is _cov_call else [(3, 11), (0, 5)]
        rc, msg = call(s, lst, host=None)
        assert rc == -1 and b"null pointer" in msg, (who, rc, msg)
        for kw in (dict(d_ws=None), dict(d_status=None)):
            rc, msg = call(s, lst, **kw)
            assert rc == -1 and b"null pointer" in msg, (who, kw, rc, msg)
        rc, msg = call(s, lst, **({"d_pairs": None} if call is _cov_call else {"d_cand": None}))
        assert rc == -1 and b"null pointer" in msg
        for n in (0, -1):
            rc, msg = call(s, lst, n=n)
            assert rc == -1 and b"count" in msg, (who, n, rc, msg)
        for bad in ([(0, 12)], [(3, 11), (-1, 2)], [(12, 0)]):
            rc, msg = call(s, bad)
            assert rc == -1 and b"out of range" in msg, (who, bad, rc, msg)
        for tol in (-1e-9, 1.0, 2.0, float("nan"), float("inf")):
            rc, msg = call(s, lst, rank_tol=tol)
            assert rc == -1 and b"rank_tol" in msg, (who, tol, rc, msg)
        # the workspace of the request's distinct columns: one too short, then exactly enough
        n_cols = 2
        need = int(lib.slam_pg_cov_workspace_len(12, n_cols))
        rc, msg = call(s, lst, ws_len=need - 1)
        assert rc == -3 and b"workspace" in msg, (who, rc, msg)
        rc, msg = call(s, lst[1:] if call is _cov_call else [(0, 5)], ws_len=int(lib.slam_pg_cov_workspace_len(12, 1)) - 1)
        assert rc == -3 and b"workspace" in msg
        # everything pg_check refuses
        rc = (lib.slam_pg_covariance(None, 0x1000, 0x1000, 1, RANK_TOL, 0x1000, 0x1000, 1 << 40, 0x1000, None)
              if call is _cov_call else
              lib.slam_pg_gate(None, 0x1000, 0x1000, 0x1000, None, 1, RANK_TOL, 0x1000, None, None, 0x1000, 1 << 40,
                               0x1000, None))
        assert rc == -1 and b"null problem" in lib.slam_last_error()
        for field in ("edge_ij", "sched", "sched_host", "ws", "state"):
            s2, e2, sc2 = tp._host_problem()
            setattr(s2, field, None)
            rc, msg = call(s2, lst)
            assert rc == -1 and b"null buffer" in msg, (who, field)
        s2, e2, sc2 = tp._host_problem()
        s2.ws_len -= 1
        rc, msg = call(s2, lst)
        assert rc == -3 and b"workspace" in msg
        s2, e2, sc2 = tp._host_problem()
        sc2[5] += 1
        rc, msg = call(s2, lst)
        assert rc == -1 and b"schedule" in msg
    rc, msg = _cov_call(s, ok, d_cov=None)
    assert rc == -1 and b"null pointer" in msg
    rc, msg = _gate_call(s, [(4, 4)])
    assert rc == -1 and b"to itself" in msg
    rc, msg = _gate_call(s, [(3, 11)], d_meas=None)
    assert rc == -1 and b"null pointer" in msg
    rc, msg = _gate_call(s, [(3, 11)], outs=(None, None, None))
    assert rc == -1 and b"null outputs" in msg


def test_python_cov_argument_checks():
    """ValueError before any device call: the methods on an object that has no
    device state at all."""
    from slam355 import posegraph as pg

    g = object.__new__(pg.PoseGraph)
    g.N = 12
    for kw in (dict(poses=[12]), dict(poses=[-1]), dict(poses=[]), dict(poses=[[0, 1]]), dict(poses=[0.0]),
               dict(pairs=[(0, 12)]), dict(pairs=[0, 1]), dict(pairs=np.zeros((0, 2), np.int32)),
               dict(pairs=[(0.0, 1.0)]), dict(rank_tol=1.0), dict(rank_tol=-1e-3), dict(rank_tol=float("nan"))):
        with pytest.raises(ValueError):
            g.covariance(**kw)
    z = np.zeros((1, 6))
    for args, kw in ((([(0, 0)], z), {}), (([(0, 12)], z), {}), (([(0, 1)], np.zeros((2, 6))), {}),
                     (([(0, 1)], z), dict(information=np.eye(6)[None], sqrt_information=np.eye(6)[None])),
                     (([(0, 1)], z), dict(rank_tol=1.0)), (([(0, 1)], z), dict(chi2=0.0)),
                     (([(0, 1)], np.full((1, 6), np.nan)), {}),
                     (([(0, 1)], z), dict(sqrt_information=np.full((1, 6, 6), np.inf)))):
        with pytest.raises(ValueError):
            g.gate(*args, **kw)
    with pytest.raises(np.linalg.LinAlgError):
        g.gate([(0, 1)], z, information=-np.eye(6)[None])
    for bad in ([(3, 3)], [(0, 12)], []):
        with pytest.raises(ValueError):
            g.relative_covariance(bad)
    assert pg.CHI2_6_99 == CHI2
    from scipy.stats import chi2 as chi2_dist

    assert abs(chi2_dist.ppf(0.99, 6) - CHI2) <= 1e-12


def test_first_order_propagation_jacobians():
    """J_i, J_j of the restatement at z = 0 are the derivatives of relative_pose."""
    rng = np.random.default_rng(8)
    for _ in range(5):
        xi = np.concatenate([rng.normal(0, 0.6, 3), rng.normal(0, 2.0, 3)])
        xj = np.concatenate([rng.normal(0, 0.6, 3), rng.normal(0, 2.0, 3)])
        _, Ji, Jj = tp.edge_jacobian(xi, xj, np.zeros(6))
        h = 1e-6
        for c in range(6):
            d = np.zeros(6)
            d[c] = h
            ni = (tp.relative_pose(xi + d, xj) - tp.relative_pose(xi - d, xj)) / (2 * h)
            nj = (tp.relative_pose(xi, xj + d) - tp.relative_pose(xi, xj - d)) / (2 * h)
            assert np.max(np.abs(Ji[:, c] - ni)) <= 2e-8 * max(1.0, np.max(np.abs(ni)))
            assert np.max(np.abs(Jj[:, c] - nj)) <= 2e-8 * max(1.0, np.max(np.abs(nj)))


@pytest.mark.parametrize("name", ["n4", "n12", "n45loop"])
def test_rank_conditions_hold_on_the_reference(name):
    """rank_tol = 1e-8 separates the gauged from the ungauged H0 by orders each way."""
    xt, edges, meas, info, A, odo = graph(name)
    H, _, _, _ = tp.dense_system(odo, edges, meas, A, None)
    free = ~tp.held_mask(tp.fixed_words(len(xt)), len(xt)).ravel()
    Hg = tp.dense_system(odo, edges, meas, A, tp.fixed_words(len(xt)))[0][np.ix_(free, free)]
    r0, r1 = pivot_ratio(H), pivot_ratio(Hg)
    print(f"{name}: ungauged pivot ratio {r0:.2e}, gauged {r1:.2e}")
    assert r0 <= 1e-3 * RANK_TOL and r1 >= 1e3 * RANK_TOL


@pytest.mark.parametrize("name", list(CANDS))
def test_gate_conditions_hold_on_the_reference(name):
    """Good candidates pass and wrong ones fail the 0.99 gate on the reference."""
    xt, edges, meas, info, A, odo = graph(name)
    x, cands, cA, good, wrong = gate_inputs(name)
    S, spread = sigma_reference(x, edges, meas, GATE_SCALE * A, tp.fixed_words(len(xt)))
    _, _, dg, cg = gate_reference(x, S, cands, good, cA)
    _, _, dw, cw = gate_reference(x, S, cands, wrong, cA)
    print(f"{name}: good d2 {np.round(dg, 2)}, wrong d2 {np.round(dw, 1)}, cond S {np.round(cg, 1)}, spread {spread:.1e}")
    assert np.all(dg < CHI2) and np.all(dw > CHI2)


# ----------------------------------------------------------------------------- GPU
def _pg(name, x, words="default", loss="linear", scale=1.0, **kw):
    from slam355 import posegraph as pg

    xt, edges, meas, info, A, odo = graph(name)
    if isinstance(words, str):
        words = tp.fixed_words(len(xt))
    if "sqrt_information" not in kw:
        kw["sqrt_information"] = scale * A
    # (copies: the shared inputs are read-only)
    return pg.PoseGraph(np.array(x), edges.copy(), meas.copy(), fixed=words, loss=loss, f_scale=loss_delta(loss), **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _worst(cov, S, req):
    return max(block_dev(cov[q], S, int(a), int(b)) for q, (a, b) in enumerate(req))


@pytest.mark.gpu
@pytest.mark.parametrize("loss", ["linear", "cauchy"])
@pytest.mark.parametrize("which", ["odo", "conv"])
@pytest.mark.parametrize("name", NAMES)
def test_gpu_blocks_match_reference(name, which, loss):
    xt, edges, meas, info, A, odo = graph(name)
    x = point(name, which, loss)
    words = tp.fixed_words(len(xt))
    S, spread = sigma_reference(x, edges, meas, A, words, loss, loss_delta(loss))
    g = _pg(name, x, loss=loss)
    req = request(name)
    cov = g.covariance(pairs=req)
    dev = _worst(cov, S, req)
    print(f"{name} {which} {loss}: deviation {dev:.2e}, spread {spread:.2e}, bar {MARGIN * spread:.2e}")
    assert np.all(np.isfinite(cov)) and g.cov_status() == 0
    assert dev <= MARGIN * spread
    if loss == "linear" and which == "odo":  # the default request: every pose's own block
        N = len(xt)
        own = g.covariance()
        assert own.shape == (N, 6, 6) and np.array_equal(_bits(own), _bits(cov[:N]))
        mixed = g.covariance(poses=[N - 1, 0], pairs=[(0, N - 1)])
        assert np.array_equal(_bits(mixed[0]), _bits(cov[N - 1])) and np.all(mixed[1] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n12", "n45loop", "n95"])
def test_gpu_exactness(name):
    xt, edges, meas, info, A, odo = graph(name)
    N = len(xt)
    g = _pg(name, odo)
    req = request(name)
    cov = g.covariance(pairs=req)
    again = g.covariance(pairs=req)
    assert np.array_equal(_bits(cov), _bits(again))  # two calls
    for q in range(N):  # a pose's own block equals its transpose
        assert np.array_equal(_bits(cov[q]), _bits(cov[q].T))
    rev = g.covariance(pairs=req[::-1])[::-1]  # the order of the request
    assert np.array_equal(_bits(cov), _bits(rev))
    flipped = g.covariance(pairs=req[:, ::-1])  # block (b, a) is block (a, b) transposed
    assert np.array_equal(_bits(flipped), _bits(cov.transpose(0, 2, 1)))
    for q in (N + len(edges) - 1, N + len(edges), N + len(edges) + 1, len(req) - 3, N // 2):  # a row asked alone
        alone = g.covariance(pairs=req[q:q + 1])
        assert np.array_equal(_bits(alone[0]), _bits(cov[q])), (q, req[q])
    assert np.array_equal(_bits(cov[-1]), _bits(cov[N]))  # the repeated entry
    assert np.array_equal(_bits(cov[-2]), _bits(cov[-3].T))  # the pair in both orders
    for q, (a, b) in enumerate(req):  # pose 0 held whole: +0.0 bit for bit
        if a == 0 or b == 0:
            assert np.all(_bits(cov[q]) == 0), (a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n12", "n45loop"])
def test_gpu_partly_held_pose(name):
    """Pose 3 held with word 0b000101: its held rows and columns +0.0, the rest
    the inverse of the free system."""
    xt, edges, meas, info, A, odo = graph(name)
    words = tp.fixed_words(len(xt), extra=(3, 0b000101))
    S, spread = sigma_reference(odo, edges, meas, A, words)
    g = _pg(name, odo, words=words)
    req = request(name)
    cov = g.covariance(pairs=req)
    held = [0, 2]
    for q, (a, b) in enumerate(req):
        if a == 3:
            assert np.all(_bits(cov[q][held, :]) == 0)
        if b == 3:
            assert np.all(_bits(cov[q][:, held]) == 0)
    assert np.count_nonzero(cov[3]) == 16
    dev = _worst(cov, S, req)
    print(f"{name} pose 3 partly held: deviation {dev:.2e}, bar {MARGIN * spread:.2e}")
    assert dev <= MARGIN * spread


@pytest.mark.gpu
def test_gpu_state_intact():
    """iterate(3); covariance(); gate(); iterate(3) is iterate(6) bit for bit."""
    x0 = tp.start_of("n35loops", "a")
    a, b = (tp._pg("n35loops", x0, lam0=tp.LAM0) for _ in range(2))
    a.iterate(3)
    before = (a.poses(), a.t["state"].cpu().numpy())
    cov = a.covariance()
    out = a.gate([(2, 30), (33, 1)], np.zeros((2, 6)), information=np.tile(np.eye(6), (2, 1, 1)))
    assert np.all(np.isfinite(cov)) and np.all(np.isfinite(out["d2"]))
    after = (a.poses(), a.t["state"].cpu().numpy())
    assert np.array_equal(_bits(before[0]), _bits(after[0])) and np.array_equal(_bits(before[1]), _bits(after[1]))
    a.iterate(3)
    b.iterate(6)
    assert b.state()["NACCEPT"] >= 1 and len(after[1]) == 20
    assert np.array_equal(_bits(a.poses()), _bits(b.poses()))
    assert np.array_equal(_bits(a.t["state"].cpu().numpy()), _bits(b.t["state"].cpu().numpy()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n4", "n12", "n45loop"])
def test_gpu_no_gauge_is_refused(name):
    xt, edges, meas, info, A, odo = graph(name)
    H = tp.dense_system(odo, edges, meas, A, None)[0]
    assert pivot_ratio(H) <= 1e-3 * RANK_TOL  # the condition on the input
    g = _pg(name, odo, words=None)
    cov = g.covariance(device=True).cpu().numpy()
    assert g.cov_status() == 1 and np.all(np.isnan(cov))
    with pytest.raises(np.linalg.LinAlgError, match="gauge"):
        g.covariance()
    with pytest.raises(np.linalg.LinAlgError, match="gauge"):
        g.gate([(0, 1)], np.zeros((1, 6)))
    g.iterate(2)  # the LM goes on as before
    assert g.state()["CHOL_FAIL"] == 0.0


@pytest.mark.gpu
def test_gpu_overflowing_information_is_refused():
    """Square-root information of 1e200: H overflows, the first pivot is not
    finite; status 1, NaN, a clean return."""
    xt, edges, meas, info, A, odo = graph("n35loops")
    g = _pg("n35loops", odo, sqrt_information=1e200 * A)
    cov = g.covariance(device=True).cpu().numpy()
    assert g.cov_status() == 1 and np.all(np.isnan(cov))
    with pytest.raises(np.linalg.LinAlgError):
        g.covariance(pairs=[(3, 30)])
    assert np.array_equal(_bits(g.poses()), _bits(odo))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n35chain", "n45loop"])
def test_gpu_full_profile_gives_the_same_blocks(name):
    xt, edges, meas, info, A, odo = graph(name)
    S, spread = sigma_reference(odo, edges, meas, A, tp.fixed_words(len(xt)))
    req = request(name)
    full = _pg(name, odo, _full_profile=True)
    T = (len(xt) + 9) // 10
    assert full.n_tiles == T * (T + 1) // 2
    dev = _worst(full.covariance(pairs=req), S, req)
    print(f"{name} full profile: deviation {dev:.2e}, bar {MARGIN * spread:.2e}")
    assert dev <= MARGIN * spread


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CANDS))
def test_gpu_gate(name):
    xt, edges, meas, info, A, odo = graph(name)
    x, cands, cA, good, wrong = gate_inputs(name)
    words = tp.fixed_words(len(xt))
    S, spread = sigma_reference(x, edges, meas, GATE_SCALE * A, words)
    bar = MARGIN * spread
    g = _pg(name, x, scale=GATE_SCALE)
    for tag, zs in (("good", good), ("wrong", wrong)):
        re, rP, rd2, cond = gate_reference(x, S, cands, zs, cA)
        assert np.all(rd2 < CHI2) if tag == "good" else np.all(rd2 > CHI2)  # on the reference first
        out = g.gate(cands, zs, sqrt_information=cA)
        de = tp._rel(out["e"], re)
        dP = max(measure(out["P"][k], rP[k]) for k in range(len(cands)))
        dd = np.abs(out["d2"] - rd2) / rd2
        print(f"{name} {tag}: e {de:.1e}, P {dP:.2e} (bar {bar:.2e}), d2 {np.round(out['d2'], 3)} ref {np.round(rd2, 3)} "
              f"rel {np.max(dd):.2e}, cond S {np.round(cond, 1)}")
        assert de <= 1e-9
        assert dP <= bar
        assert np.all(dd <= cond * bar)
        assert np.array_equal(out["accept"], rd2 <= CHI2) and g.gate_undetermined() == 0
        for k in range(len(cands)):
            assert np.array_equal(_bits(out["P"][k]), _bits(out["P"][k].T))
        info_form = g.gate(cands, zs, information=np.stack([a.T @ a for a in cA]))
        assert np.allclose(info_form["d2"], out["d2"], rtol=1e-9)
    # the relative-pose covariance: the gate's P with zero measurements and no information
    rel = g.relative_covariance(cands)
    zero = g.gate(cands, np.zeros((len(cands), 6)))
    assert np.array_equal(_bits(rel), _bits(zero["P"]))
    _, rP, _, _ = gate_reference(x, S, cands, np.zeros((len(cands), 6)), None)
    dP = max(measure(rel[k], rP[k]) for k in range(len(cands)))
    print(f"{name} relative covariance: {dP:.2e} (bar {bar:.2e})")
    assert dP <= bar


@pytest.mark.gpu
def test_gpu_gate_of_two_held_poses_is_undetermined():
    xt, edges, meas, info, A, odo = graph("n12")
    g = _pg("n12", odo, words=tp.fixed_words(12, extra=(5, 0x3F)))
    out = g.gate([(0, 5), (5, 0), (2, 9)], np.zeros((3, 6)))
    assert np.isnan(out["d2"][0]) and np.isnan(out["d2"][1]) and np.isfinite(out["d2"][2])
    assert g.cov_status() == 0 and g.gate_undetermined() == 2
    assert np.all(_bits(out["P"][:2]) == 0) and not np.any(out["accept"][:2])
    one = g.gate([(0, 5)], np.zeros((1, 6)))
    assert np.isnan(one["d2"][0]) and int(g._cov_status[1].item()) == 1
    with_info = g.gate([(0, 5)], np.zeros((1, 6)), information=np.eye(6)[None])  # R alone carries it
    assert np.isfinite(with_info["d2"][0]) and g.gate_undetermined() == 0
