"""Landmark and landmark-camera covariance blocks (slam_ba_covariance_points,
slam355.ba.cov_points / cov_cross, BAProblem.point_covariance /
reprojection_covariance, BABatch.point_covariance).

Semantics: with J~ the clamped, masked, robust-weighted Jacobian of the LM
steps at the live parameters and H = J~^T J~ (no damping) over the free
parameters, the call returns the 3x3 point blocks Sigma_pp, the 3x9
point-camera blocks Sigma_pc and the 9x9 camera blocks Sigma_cc of H^-1.

Reference: NumPy on oracle.ba.residual_and_jacobian, by two routes -- (i) the
blocks of np.linalg.inv of the full free H; (ii) per-point np.linalg.inv(V),
S0, its Cholesky inverse, then
  Sigma_pp = V^-1 + V^-1 (W^T Sigma_cc W) V^-1,  Sigma_pc = -V^-1 W^T Sigma_cc.
Error measure (correlation-scaled): |d| / sqrt(Sigma_ii Sigma_jj), the diagonal
from route (i).

Bar of every GPU comparison: 100 x the problem's own two-route spread, computed
at run time, separately for pp, pc and cc (the kernel's formula -- cofactor
V^-1, the sandwich with a Sigma_cc that is not LAPACK's -- emulated on the CPU
deviates from route (i) by 1 .. 6 x the spread, the GPU's Sigma_cc by up to
2.3 x; a dropped observation pair, a wrong mirror or a missed held column shows
at 1e-3 .. 1).  Condition on the reference (a host test): each spread <= 1e-9.

Problems: slam355.synthetic.ba_problem seed 3 at 6x150x4, 10x300x4, 15x400x4
(packed sys, blocks straddling tiles), 30x900x5 (absent blocks), cameras 0 and
1 held whole; and "deep": 10x300x4 with points 0..4 observed by every camera
(10 observations: 100 ordered pairs > 64 lanes, two chunks of 8, slot mode).
"""
import ctypes

import numpy as np
import pytest

from oracle import ba as oba

SHAPES = {"6x150": (6, 150, 4), "10x300": (10, 300, 4), "15x400": (15, 400, 4), "30x900": (30, 900, 5)}
SPREAD_MAX = 1e-9  # condition on the reference's two routes
MARGIN = 100.0
ST_SLOTS = ("LAMBDA", "NU", "COST", "COST_NEW", "RHO", "NACCEPT", "CHOL_FAIL")

_PROBLEMS, _REFS = {}, {}


def problem(shape):
    """(cams, pts, ci, pi, qs) of ba_problem seed 3 (or the deep-row variant), shared and never written."""
    if shape not in _PROBLEMS:
        from slam355.synthetic import ba_problem, bal_project

        if shape == "deep":
            cams, pts, ci, pi, qs = problem("10x300")
            C = len(cams)
            keep = pi >= 5
            dci, dpi = np.tile(np.arange(C), 5), np.repeat(np.arange(5), C)
            dq = bal_project(pts[dpi], cams[dci]) + np.random.default_rng(11).normal(0, 0.5, (5 * C, 2))
            pr = (cams, pts, np.concatenate([ci[keep], dci]), np.concatenate([pi[keep], dpi]),
                  np.concatenate([qs[keep], dq]))
        else:
            pr = ba_problem(np.random.default_rng(3), *SHAPES[shape])
        for a in pr:
            a.setflags(write=False)
        _PROBLEMS[shape] = pr
    return _PROBLEMS[shape]


def gauge(C, intr_held, anchors=2):
    """[C, 9] 0/1: the first `anchors` cameras held whole, the others' f, k1, k2 held or free."""
    fx = np.zeros((C, 9), np.uint8)
    fx[:anchors] = 1
    if intr_held:
        fx[:, 6:] = 1
    return fx


def request(C):
    """The camera request of test_ba_cov: all marginal blocks plus the pairs (2,3), (3,2), (2,C-1), (0,2)."""
    return dict(cameras=np.arange(C), pairs=[(2, 3), (3, 2), (2, C - 1), (0, 2)])


def cross_request(C, P):
    """Points {0, 1, P-1} x every camera: held, non-observing and the last camera included."""
    return np.array([(p, c) for p in (0, 1, P - 1) for c in range(C)])


class Ref:
    """Route (i) blocks (cc [9C, 9C], pc [P, 3, 9C], pp [P, 3, 3]; zeros on held
    camera rows / columns), sqrt of its diagonal (dc [9C], dp [P, 3]) and the
    three correlation-scaled spreads between routes (i) and (ii)."""


def weighted_jacobian(cams, pts, ci, pi, qs, loss=None, delta=1.0):
    r, J = oba.residual_and_jacobian(cams, pts, ci, pi, qs)
    if loss is not None:  # sqrt(w), w = rho'(z), z = |r|^2 / delta^2 of the clamped residual
        z = np.sum(r * r, axis=1) / delta ** 2
        w = {"cauchy": 1.0 / (1.0 + z), "soft_l1": 1.0 / np.sqrt(1.0 + z),
             "huber": np.where(z > 1.0, 1.0 / np.sqrt(np.maximum(z, 1.0)), 1.0)}[loss]
        J = J * np.sqrt(w)[:, None, None]
    return J


def reference(cams, pts, ci, pi, qs, fixed, loss=None, delta=1.0):
    C, P = len(cams), len(pts)
    J = weighted_jacobian(cams, pts, ci, pi, qs, loss, delta)
    n = 9 * C + 3 * P
    idx = np.concatenate([(9 * ci)[:, None] + np.arange(9), (9 * C + 3 * pi)[:, None] + np.arange(3)], 1)
    H = np.zeros((n, n))
    np.add.at(H, (idx[:, :, None], idx[:, None, :]), np.einsum("oai,oaj->oij", J, J))
    free_c = np.nonzero(np.asarray(fixed).reshape(-1) == 0)[0]
    free = np.concatenate([free_c, 9 * C + np.arange(3 * P)])
    nc = len(free_c)
    Hf = H[np.ix_(free, free)]
    s1 = np.linalg.inv(Hf)  # route (i)
    U, W = Hf[:nc, :nc], Hf[:nc, nc:].reshape(nc, P, 3)
    V = Hf[nc:, nc:].reshape(P, 3, P, 3)[np.arange(P), :, np.arange(P), :]
    Vi = np.linalg.inv(V)  # route (ii)
    S0 = U - np.einsum("cpi,pij->cpj", W, Vi).reshape(nc, 3 * P) @ W.reshape(nc, 3 * P).T
    Li = np.linalg.inv(np.linalg.cholesky(0.5 * (S0 + S0.T)))
    cc2 = Li.T @ Li
    pc2 = -np.einsum("pij,cpj,cd->pid", Vi, W, cc2)
    pp2 = Vi - np.einsum("pid,dpj,pjk->pik", pc2, W, Vi)
    d = np.sqrt(np.diag(s1))
    dcf, dp = d[:nc], d[nc:].reshape(P, 3)
    pp1 = s1[nc:, nc:].reshape(P, 3, P, 3)[np.arange(P), :, np.arange(P), :]
    pc1 = s1[nc:, :nc].reshape(P, 3, nc)
    ref = Ref()
    ref.spread = dict(cc=float(np.max(np.abs(s1[:nc, :nc] - cc2) / np.outer(dcf, dcf))),
                      pc=float(np.max(np.abs(pc1 - pc2) / (dp[:, :, None] * dcf[None, None, :]))),
                      pp=float(np.max(np.abs(pp1 - pp2) / (dp[:, :, None] * dp[:, None, :]))))
    ref.cc = np.zeros((9 * C, 9 * C))
    ref.cc[np.ix_(free_c, free_c)] = s1[:nc, :nc]
    ref.pc = np.zeros((P, 3, 9 * C))
    ref.pc[:, :, free_c] = pc1
    ref.pp, ref.dp = pp1.copy(), dp
    ref.dc = np.zeros(9 * C)
    ref.dc[free_c] = dcf
    for a in (ref.cc, ref.pc, ref.pp, ref.dp, ref.dc):
        a.setflags(write=False)
    return ref


def shape_reference(shape, intr_held):
    key = (shape, intr_held)
    if key not in _REFS:
        pr = problem(shape)
        _REFS[key] = reference(*pr, gauge(len(pr[0]), intr_held))
    return _REFS[key]


def deviations(ref, got, pts, cross, pairs):
    """Largest correlation-scaled |got - reference| of the three outputs, free entries only."""
    pts, cross, pairs = np.asarray(pts), np.asarray(cross).reshape(-1, 2), np.asarray(pairs).reshape(-1, 2)
    dev = dict(pp=0.0, pc=0.0, cc=0.0)
    if len(pts):
        dev["pp"] = float(np.max(np.abs(got.points - ref.pp[pts]) / (ref.dp[pts][:, :, None] * ref.dp[pts][:, None, :])))
    for blk, (p, c) in zip(got.cross, cross):
        sc = np.outer(ref.dp[p], ref.dc[9 * c:9 * c + 9])
        m = sc > 0
        if m.any():
            dev["pc"] = max(dev["pc"], float(np.max(np.abs(blk - ref.pc[p][:, 9 * c:9 * c + 9])[m] / sc[m])))
    for blk, (a, b) in zip(got.cameras, pairs):
        sc = np.outer(ref.dc[9 * a:9 * a + 9], ref.dc[9 * b:9 * b + 9])
        m = sc > 0
        if m.any():
            dev["cc"] = max(dev["cc"], float(np.max(np.abs(blk - ref.cc[9 * a:9 * a + 9, 9 * b:9 * b + 9])[m] / sc[m])))
    return dev


def check_bars(label, ref, dev):
    for k in ("pp", "pc", "cc"):
        print(f"{label} {k}: deviation {dev[k]:.2e}, spread {ref.spread[k]:.2e}, bar {MARGIN * ref.spread[k]:.2e}")
    for k in ("pp", "pc", "cc"):
        assert ref.spread[k] <= SPREAD_MAX, k
        assert dev[k] <= MARGIN * ref.spread[k], k


def check_structure(got, cross, fixed):
    """pp bitwise symmetric with a positive diagonal; pc columns of held parameters +0.0."""
    assert got.points.dtype == got.cross.dtype == got.cameras.dtype == np.float64
    assert got.points.shape[1:] == (3, 3) and got.cross.shape[1:] == (3, 9) and got.cameras.shape[1:] == (9, 9)
    assert np.all(np.isfinite(got.points)) and np.all(np.isfinite(got.cross))
    assert np.array_equal(got.points.view(np.uint64), got.points.transpose(0, 2, 1).copy().view(np.uint64))
    assert np.all(got.points[:, np.arange(3), np.arange(3)] > 0.0)
    for blk, (p, c) in zip(got.cross, np.asarray(cross).reshape(-1, 2)):
        held = fixed[c] != 0
        assert np.all(blk[:, held] == 0.0) and not np.any(np.signbit(blk[:, held]))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ----------------------------------------------------------------------------- host
def test_cov_points_and_cross_accept():
    from slam355 import ba

    p = ba.cov_points(5)
    assert p.dtype == np.int32 and p.flags.c_contiguous and p.tolist() == [0, 1, 2, 3, 4]
    assert ba.cov_points(5, [4, 0, 4]).tolist() == [4, 0, 4]  # a repeat is kept
    assert ba.cov_points(5, np.array([2], np.int64)).dtype == np.int32
    assert ba.cov_points(5, []).shape == (0,) and ba.cov_points(0).shape == (0,)
    c = ba.cov_cross(5, 3, [(4, 2), (0, 0), (4, 2)])
    assert c.dtype == np.int32 and c.flags.c_contiguous and c.tolist() == [[4, 2], [0, 0], [4, 2]]
    assert ba.cov_cross(5, 3, None).shape == (0, 2) and ba.cov_cross(5, 3, []).shape == (0, 2)
    assert ba.cov_cross(5, 3, np.array([[1, 2]], np.int16)).tolist() == [[1, 2]]
    assert ba.cov_cross(2, 7, [(1, 6)]).tolist() == [[1, 6]]  # the bounds are per column
    assert ba.PointCovariance._fields == ("points", "cross", "cameras")


@pytest.mark.parametrize("pts", [[5], [-1], [[0, 1]], [0.5], [True], ["a"], 3])
def test_cov_points_rejects(pts):
    from slam355 import ba

    with pytest.raises(ValueError):
        ba.cov_points(5, pts)
    with pytest.raises(ValueError):
        ba.cov_points(-1)


@pytest.mark.parametrize("cross", [[(5, 0)], [(0, 3)], [(-1, 0)], [(0, -1)], [0, 1], [(0, 1, 2)], [(0.0, 1.0)],
                                   [(True, False)], [("a", "b")], [(3, 4)]])
def test_cov_cross_rejects(cross):
    from slam355 import ba

    with pytest.raises(ValueError):
        ba.cov_cross(5, 3, cross)
    with pytest.raises(ValueError):
        ba.cov_cross(5, 0, None)


def test_signature_of_the_new_symbol():
    from slam355 import _lib

    assert len(_lib.SIGNATURES["slam_ba_covariance_points"]) == 15
    assert _lib.lib.slam_ba_covariance_points.restype is ctypes.c_int
    assert len(_lib.SIGNATURES["slam_ba_covariance"]) == 9
    assert _lib.lib.slam_abi_version() == 1
    assert _lib.lib.slam_ba_problem_size() == 408 == ctypes.sizeof(_lib.BAProblemStruct)


@pytest.mark.parametrize("intr_held", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES) + ["deep"])
def test_reference_routes_agree(shape, intr_held):
    """The condition on the reference: its two routes agree to <= 1e-9
    (correlation-scaled) for pp, pc and cc on every GPU-test problem."""
    ref = shape_reference(shape, intr_held)
    print(f"{shape} intrinsics {'held' if intr_held else 'free'}: spreads {ref.spread}")
    assert all(v <= SPREAD_MAX for v in ref.spread.values())
    assert np.all(ref.dp > 0.0)
    fx = gauge(len(problem(shape)[0]), intr_held).reshape(-1) != 0
    assert np.all(ref.pc[:, :, fx] == 0.0) and np.all(ref.dc[~fx] > 0.0)


# ----------------------------------------------------------------------------- GPU
def run_parity(label, prob, ref, fx, C, P):
    """Every point, the cross request, the camera request: bars, structure, and
    the bit identities of sub-requests, repeats, a second call and covariance()."""
    from slam355 import ba

    cross = cross_request(C, P)
    pairs = ba.cov_pairs(C, **request(C))
    got = prob.point_covariance(cross=cross, **request(C))
    assert isinstance(got, ba.PointCovariance)
    assert len(got.points) == P and len(got.cross) == len(cross) and len(got.cameras) == len(pairs)
    assert prob.cov_status() == 0 and prob.cov_undetermined() == 0
    check_bars(label, ref, deviations(ref, got, np.arange(P), cross, pairs))
    check_structure(got, cross, fx)
    again = prob.point_covariance(cross=cross, **request(C))
    for x, y in zip(got, again):
        assert np.array_equal(bits(x), bits(y))
    sub = prob.point_covariance(points=[P - 1, 3, 3, 0], cross=[cross[C + 1], cross[2], cross[C + 1]])
    assert sub.cameras.shape == (0, 9, 9)
    assert np.array_equal(bits(sub.points), bits(got.points[[P - 1, 3, 3, 0]]))
    assert np.array_equal(bits(sub.cross), bits(got.cross[[C + 1, 2, C + 1]]))
    only = prob.point_covariance(points=[], cameras=[2])
    assert only.points.shape == (0, 3, 3) and only.cross.shape == (0, 3, 9)
    assert np.array_equal(bits(only.cameras), bits(got.cameras[[2]]))
    assert np.array_equal(bits(got.cameras), bits(prob.covariance(**request(C))))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("shape,intr_held,lin_mode", [("6x150", False, "auto"), ("6x150", False, "slot"),
                                                      ("10x300", False, "auto"), ("15x400", False, "auto"),
                                                      ("30x900", True, "auto")])
def test_gpu_point_covariance_matches_reference(shape, intr_held, lin_mode):
    from slam355 import ba

    pr = problem(shape)
    C, P = len(pr[0]), len(pr[1])
    fx = gauge(C, intr_held)
    prob = ba.BAProblem(*pr, fixed=fx, lin_mode=lin_mode)
    assert prob.lin_mode == ("slot" if lin_mode == "slot" else "mfma")
    run_parity(f"{shape} intrinsics {'held' if intr_held else 'free'} {prob.lin_mode}", prob,
               shape_reference(shape, intr_held), fx, C, P)


@pytest.mark.gpu
def test_gpu_point_covariance_deep_rows():
    """Points 0..4 seen by all 10 cameras: 100 ordered observation pairs per point (two chunks), slot mode."""
    from slam355 import ba

    pr = problem("deep")
    C, P = len(pr[0]), len(pr[1])
    assert np.all(np.bincount(pr[3], minlength=P)[:5] == C)
    fx = gauge(C, False)
    prob = ba.BAProblem(*pr, fixed=fx)
    assert prob.lin_mode == "slot"
    run_parity("deep 10x300", prob, shape_reference("deep", False), fx, C, P)


@pytest.mark.gpu
def test_gpu_point_covariance_at_live_parameters():
    """After iterate(3) the blocks are those of the reference at exactly params()."""
    from slam355 import ba
    from slam355.synthetic import perturb

    cams, pts, ci, pi, qs = problem("15x400")
    C, P = len(cams), len(pts)
    fx = gauge(C, False)
    prob = ba.BAProblem(*perturb(np.random.default_rng(5), cams, pts), ci, pi, qs, fixed=fx)
    prob.iterate(3)
    assert prob.state()["NACCEPT"] >= 1
    lc, lp = prob.params()
    assert not np.array_equal(lc, cams)
    ref = reference(lc, lp, ci, pi, qs, fx)
    cross = cross_request(C, P)
    got = prob.point_covariance(cross=cross, **request(C))
    check_bars("live 15x400", ref, deviations(ref, got, np.arange(P), cross, ba.cov_pairs(C, **request(C))))
    check_structure(got, cross, fx)


@pytest.mark.gpu
def test_gpu_point_covariance_robust():
    """loss = cauchy, f_scale 1.5, 10 % of the observations displaced by up to
    +-60 px: the blocks are those of the sqrt(w)-weighted Jacobian."""
    from slam355 import ba

    cams, pts, ci, pi, qs = problem("10x300")
    C, P = len(cams), len(pts)
    rng = np.random.default_rng(11)
    out = rng.random(len(qs)) < 0.1
    qs = qs.copy()
    qs[out] += rng.uniform(-60, 60, (int(out.sum()), 2))
    fx = gauge(C, False)
    ref = reference(cams, pts, ci, pi, qs, fx, "cauchy", 1.5)
    plain = reference(cams, pts, ci, pi, qs, fx)
    assert np.max(np.abs(plain.pp - ref.pp) / (ref.dp[:, :, None] * ref.dp[:, None, :])) > 1e-2  # the weights matter
    prob = ba.BAProblem(cams, pts, ci, pi, qs, fixed=fx, loss="cauchy", f_scale=1.5)
    cross = cross_request(C, P)
    got = prob.point_covariance(cross=cross, **request(C))
    check_bars("cauchy 10x300", ref, deviations(ref, got, np.arange(P), cross, ba.cov_pairs(C, **request(C))))
    check_structure(got, cross, fx)


@pytest.mark.gpu
def test_gpu_point_covariance_all_cameras_held():
    """Every camera held whole: pc all +0.0, pp = V^-1 within 100 x the spread
    between np.linalg.inv(V) and the Cholesky inverse of V, camera status 0."""
    from slam355 import ba

    cams, pts, ci, pi, qs = problem("10x300")
    C, P = len(cams), len(pts)
    fx = np.ones((C, 9), np.uint8)
    J = weighted_jacobian(cams, pts, ci, pi, qs)[:, :, 9:]
    V = np.zeros((P, 3, 3))
    np.add.at(V, pi, np.einsum("oai,oaj->oij", J, J))
    v1 = np.linalg.inv(V)
    Li = np.linalg.inv(np.linalg.cholesky(V))
    v2 = Li.transpose(0, 2, 1) @ Li
    d = np.sqrt(v1[:, np.arange(3), np.arange(3)])
    sc = d[:, :, None] * d[:, None, :]
    spread = float(np.max(np.abs(v1 - v2) / sc))
    assert spread <= SPREAD_MAX
    prob = ba.BAProblem(cams, pts, ci, pi, qs, fixed=fx)
    cross = cross_request(C, P)
    got = prob.point_covariance(cross=cross, cameras=[0, C - 1])
    assert prob.cov_status() == 0 and prob.cov_undetermined() == 0
    dev = float(np.max(np.abs(got.points - v1) / sc))
    print(f"all held 10x300 pp: deviation {dev:.2e}, spread {spread:.2e}, bar {MARGIN * spread:.2e}")
    assert dev <= MARGIN * spread
    assert np.all(got.cross == 0.0) and not np.any(np.signbit(got.cross))
    assert np.all(got.cameras == 0.0)
    check_structure(got, cross, fx)


@pytest.mark.gpu
def test_gpu_point_covariance_unobserved_point():
    """An appended point without an observation: its rows are NaN and counted,
    the camera status stays 0, nothing is raised, every other row keeps its bar."""
    from slam355 import ba

    cams, pts, ci, pi, qs = problem("10x300")
    C, P = len(cams), len(pts)
    fx = gauge(C, False)
    ref = shape_reference("10x300", False)
    prob = ba.BAProblem(cams, np.concatenate([pts, [[0.3, -0.2, -20.0]]]), ci, pi, qs, fixed=fx)
    assert prob.P == P + 1
    cross = np.concatenate([cross_request(C, P), [(P, 2), (P, 0), (P, 2)]])
    got = prob.point_covariance(cross=cross, **request(C))
    assert prob.cov_status() == 0
    assert prob.cov_undetermined() == 1 + 3
    assert np.all(np.isnan(got.points[P])) and np.all(np.isnan(got.cross[-3:]))
    seen = ba.PointCovariance(got.points[:P], got.cross[:-3], got.cameras)
    check_bars("10x300 + unobserved point", ref,
               deviations(ref, seen, np.arange(P), cross[:-3], ba.cov_pairs(C, **request(C))))
    check_structure(seen, cross[:-3], fx)
    only = prob.point_covariance(points=[P, 0, P])
    assert prob.cov_undetermined() == 2 and np.array_equal(bits(only.points[1]), bits(got.points[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("graphed", [False, True])
@pytest.mark.parametrize("shape", ["6x150", "15x400"])
def test_gpu_point_covariance_has_no_side_effects(shape, graphed):
    """iterate(3); point_covariance(); iterate(3) equals iterate(6) on a twin:
    the parameters and the LM state slots bit for bit."""
    from slam355 import ba
    from slam355.synthetic import perturb

    cams, pts, ci, pi, qs = problem(shape)
    C, P = len(cams), len(pts)
    fx = gauge(C, False)
    start = perturb(np.random.default_rng(5), cams, pts)
    a = ba.BAProblem(*start, ci, pi, qs, fixed=fx)
    b = ba.BAProblem(*start, ci, pi, qs, fixed=fx)
    step = (lambda p, n: p.iterate_graphed(n)) if graphed else (lambda p, n: p.iterate(n))
    step(a, 3)
    before = a.state()
    a.point_covariance(cross=cross_request(C, P), **request(C))
    after = a.state()
    assert all(np.float64(before[k]).tobytes() == np.float64(after[k]).tobytes() for k in before)
    step(a, 3)
    step(b, 6)
    sa, sb = a.state(), b.state()
    assert sa["NACCEPT"] >= 2
    for k in ST_SLOTS:
        assert np.float64(sa[k]).tobytes() == np.float64(sb[k]).tobytes(), k
    for x, y in zip(a.params(), b.params()):
        assert np.array_equal(bits(x), bits(y))


@pytest.mark.gpu
def test_gpu_point_covariance_reports_rank_deficiency():
    """Only camera 0 held: LinAlgError; device=True gives three NaN outputs and status word 0 = 1."""
    import torch
    from slam355 import ba

    pr = problem("10x300")
    C, P = len(pr[0]), len(pr[1])
    prob = ba.BAProblem(*pr, fixed=gauge(C, False, 1))
    with pytest.raises(np.linalg.LinAlgError):
        prob.point_covariance()
    out = prob.point_covariance(cross=cross_request(C, P), **request(C), device=True)
    torch.cuda.synchronize()
    assert prob.cov_status() == 1
    assert out.points.shape == (P, 3, 3) and out.cross.shape == (3 * C, 3, 9) and out.cameras.shape == (C + 4, 9, 9)
    for t in out:
        assert isinstance(t, torch.Tensor) and t.is_cuda and bool(torch.isnan(t).all())


@pytest.mark.gpu
def test_gpu_window_set_and_batch_point_covariance():
    """A BAWindowSet.build window gives the bits of the same problem built as a
    BAProblem (each maps the caller's point order through its own perm);
    BABatch.point_covariance equals the per-problem calls."""
    import torch
    from slam355 import ba

    pr = problem("10x300")
    C, P = len(pr[0]), len(pr[1])
    fx = gauge(C, True)
    s = torch.cuda.Stream()
    ws = ba.BAWindowSet()
    win = ws.build([pr], s, fixed=fx)[0]
    assert type(win).__name__ == "_WindowProblem"
    ref = ba.BAProblem(*pr, fixed=fx)
    for p in (win, ref):
        p.iterate(2)
    req = dict(points=[7, P - 1, 0, 7], cross=cross_request(C, P), cameras=[2, 3])
    got, exp = win.point_covariance(**req), ref.point_covariance(**req)
    for x, y in zip(got, exp):
        assert np.array_equal(bits(x), bits(y))
    every = win.point_covariance()
    assert np.array_equal(bits(every.points[[7, P - 1, 0, 7]]), bits(got.points))
    ws.build([pr], s, fixed=fx)
    ws.build([pr], s, fixed=fx)
    with pytest.raises(RuntimeError):
        win.point_covariance()

    specs = [("6x150", False), ("10x300", True), ("6x150", True)]
    probs = [ba.BAProblem(*problem(sh), fixed=gauge(SHAPES[sh][0], h)) for sh, h in specs]
    batch = ba.BABatch(probs)
    batch.iterate(2)
    req = dict(points=[3, 149], cross=[(3, 5), (0, 0)], pairs=[(2, 5)], scale=2.0)
    res = batch.point_covariance(**req)
    assert isinstance(res, list) and len(res) == 3
    for g, p in zip(res, probs):
        assert g.points.shape == (2, 3, 3) and g.cross.shape == (2, 3, 9) and g.cameras.shape == (1, 9, 9)
        for x, y in zip(g, p.point_covariance(**req)):
            assert np.array_equal(bits(x), bits(y))
        unit = p.point_covariance(points=[3, 149])
        assert np.all(np.abs(g.points - 2.0 * unit.points) <= 1e-15 * np.abs(2.0 * unit.points))


@pytest.mark.gpu
def test_gpu_c_abi_refusals_and_out_of_range():
    """Refusals return non-zero with a message and launch nothing (outputs and
    status keep their sentinels); an out-of-range device index gives a NaN row."""
    import torch
    from slam355 import _lib, ba

    pr = problem("6x150")
    C, P = 6, 150
    prob = ba.BAProblem(*pr, fixed=gauge(C, False))
    prob.iterate(1)
    lam = prob.state()["LAMBDA"]
    n = int(_lib.lib.slam_ba_cov_workspace_len(C))
    ws = torch.zeros(n, dtype=torch.float64, device="cuda")
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device="cuda")  # noqa: E731
    pairs, points, cross = i32([[2, 2], [9, 2]]), i32([0, P, -1, 5]), i32([[0, 2], [P, 2], [0, C], [5, 3]])
    f64 = lambda *shp: torch.full(shp, 5.0, dtype=torch.float64, device="cuda")  # noqa: E731
    cc, pp, pc, ppall = f64(2, 9, 9), f64(4, 3, 3), f64(4, 3, 9), f64(P, 3, 3)
    status = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    sp = ba.stream_ptr()
    dp = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def call(pr_=pairs, n_pr=2, cc_=cc, pt_=points, n_pt=4, pp_=pp, cr_=cross, n_cr=4, pc_=pc, tol=1e-8,
             wsp=ws, ws_len=n, st=status):
        return _lib.lib.slam_ba_covariance_points(ctypes.byref(prob._s), dp(pr_), n_pr, dp(cc_), dp(pt_), n_pt,
                                                  dp(pp_), dp(cr_), n_cr, dp(pc_), tol, dp(wsp), ws_len, dp(st), sp)

    for kw, word in ((dict(n_pr=0, n_pt=0, n_cr=0), b"nothing requested"), (dict(n_pr=-1), b"negative count"),
                     (dict(n_pt=-2), b"negative count"), (dict(n_cr=-1), b"negative count"),
                     (dict(pr_=None), b"null pointer"), (dict(cc_=None), b"null pointer"),
                     (dict(pt_=None), b"null pointer"), (dict(pp_=None), b"null pointer"),
                     (dict(cr_=None), b"null pointer"), (dict(pc_=None), b"null pointer"),
                     (dict(st=None), b"null pointer"), (dict(tol=float("nan")), b"rank_tol"),
                     (dict(tol=1.0), b"rank_tol"), (dict(tol=-1e-9), b"rank_tol"),
                     (dict(ws_len=n - 1), b"workspace"), (dict(wsp=None), b"workspace")):
        assert call(**kw) != 0, kw
        assert word in _lib.lib.slam_last_error(), (kw, _lib.lib.slam_last_error())
    torch.cuda.synchronize()
    assert status.tolist() == [7, 7] and all(bool((t == 5.0).all()) for t in (cc, pp, pc))
    assert prob.state()["LAMBDA"] == lam
    assert call() == 0  # the accepted call runs; out-of-range entries are NaN rows, not counted
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0] and prob.state()["LAMBDA"] == lam
    order = prob.perm if prob.perm is not None else np.arange(P)  # device point k = the caller's order[k]
    exp = prob.point_covariance(points=order[[0, 5]], cross=[(order[0], 2), (order[5], 3)], cameras=[2])
    got_pp, got_pc, got_cc = pp.cpu().numpy(), pc.cpu().numpy(), cc.cpu().numpy()
    assert np.all(np.isnan(got_pp[1:3])) and np.all(np.isnan(got_pc[1:3])) and np.all(np.isnan(got_cc[1]))
    assert np.array_equal(bits(got_pp[[0, 3]]), bits(exp.points))
    assert np.array_equal(bits(got_pc[[0, 3]]), bits(exp.cross))
    assert np.array_equal(bits(got_cc[0]), bits(exp.cameras[0]))
    # the all-points form: a null list with n_points == n_pts, in device order
    assert call(n_pr=0, pt_=None, n_pt=P, pp_=ppall, n_cr=0) == 0
    torch.cuda.synchronize()
    every = prob.point_covariance().points
    assert np.array_equal(bits(ppall.cpu().numpy()), bits(every[order]))
    assert call(n_pr=0, pt_=None, n_pt=P - 1, pp_=ppall, n_cr=0) != 0 and b"n_pts" in _lib.lib.slam_last_error()


@pytest.mark.gpu
def test_gpu_reprojection_covariance():
    """20 (point, camera) pairs of 10x300 against A Sigma A^T of route (i), A the
    oracle's Jacobian at q = the projection (clamp inactive), scaled by the
    reference's diagonal; bar 100 x the largest of the three spreads.  The
    pairs: 3 observing ones, the held cameras 0 and 1, the last camera, 14 drawn
    at random (seed 7).  Measured on the MI355X: deviation 4.68e-9, bar 9.12e-9
    -- A Sigma A^T cancels (point-camera correlations reach 0.99), so this is
    the tightest comparison of the file."""
    from slam355 import ba

    cams, pts, ci, pi, qs = problem("10x300")
    C, P = len(cams), len(pts)
    fx = gauge(C, False)
    ref = shape_reference("10x300", False)
    rng = np.random.default_rng(7)
    pp, cc = rng.integers(0, P, 20), rng.integers(0, C, 20)
    pp[:3], cc[:3] = pi[:3], ci[:3]      # observing pairs
    cc[3:6] = (0, 1, C - 1)              # held cameras and the last one
    proj, _ = oba.residual_and_jacobian(cams, pts, cc, pp, np.zeros((20, 2)))
    assert np.max(np.abs(proj)) < 5000.0
    r, A = oba.residual_and_jacobian(cams, pts, cc, pp, proj)
    assert np.all(r == 0.0)
    exp = np.empty((20, 2, 2))
    for k, (p, c) in enumerate(zip(pp, cc)):
        S = np.empty((12, 12))
        S[:9, :9], S[9:, 9:] = ref.cc[9 * c:9 * c + 9, 9 * c:9 * c + 9], ref.pp[p]
        S[9:, :9] = ref.pc[p][:, 9 * c:9 * c + 9]
        S[:9, 9:] = S[9:, :9].T
        exp[k] = A[k] @ S @ A[k].T
    prob = ba.BAProblem(cams, pts, ci, pi, qs, fixed=fx)
    got = prob.reprojection_covariance(pp, cc)
    assert got.shape == (20, 2, 2) and np.array_equal(bits(got), bits(got.transpose(0, 2, 1)))
    d = np.sqrt(exp[:, np.arange(2), np.arange(2)])
    dev = float(np.max(np.abs(got - exp) / (d[:, :, None] * d[:, None, :])))
    bar = MARGIN * max(ref.spread.values())
    print(f"reprojection 10x300: deviation {dev:.2e}, spreads {ref.spread}, bar {bar:.2e}")
    assert dev <= bar
    with pytest.raises(ValueError):
        prob.reprojection_covariance([0, 1], [0])
    with pytest.raises(ValueError):
        prob.reprojection_covariance([P], [0])
