"""Marginal covariance of the camera parameters (slam_ba_covariance,
slam355.ba.cov_pairs / BAProblem.covariance / BABatch.covariance).

Semantics: with J~ the clamped, masked (held columns removed), robust-weighted
Jacobian of the LM steps at the live parameters and H = J~^T J~ (no damping)
over the free parameters, the call returns 9x9 blocks of Sigma = (H^-1)_cc =
S0^-1, S0 the Schur-reduced camera system; rows and columns of held parameters
are exact zeros.

Reference: NumPy on top of oracle.ba.residual_and_jacobian, by two routes --
(i) np.linalg.inv of the full free H, camera part; (ii) per-point 3x3
inverses, the Schur complement, its Cholesky factor, L^-T L^-1.  Error measure
(correlation-scaled): |dSigma_ij| / sqrt(Sigma_ii Sigma_jj) over free entries.

Problems: slam355.synthetic.ba_problem, seed 3, at 6x150x4 (one tile, padding
inside it, dense sys), 10x300x4 (two tiles, dense sys), 15x400x4 (three tiles,
packed sys, the first trailing update i > j > k) and 30x900x5 (five tiles,
packed sys with absent blocks), cameras 0 and 1 held whole (the gauge), the
other cameras' intrinsics free or held.

Bar of every GPU comparison: 100 x that problem's own two-route spread,
computed at run time (tile order and MFMA accumulation order differ from
LAPACK's; both sides carry cond * eps error with different constants; a
dropped tile, a wrong mirror or a missed held row shows as 1e-3 .. 1).
Condition on the reference (not a measurement): the spread is <= 1e-9, so the
bar never exceeds 1e-7.  Measured here on the CPU: spread <= 2.1e-10 with the
intrinsics free, <= 9.3e-11 with them held.
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
    """(cams, pts, ci, pi, qs) of ba_problem seed 3, shared and never written."""
    if shape not in _PROBLEMS:
        from slam355.synthetic import ba_problem

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
    """All marginal blocks plus the pairs (2,3), (3,2), (2,C-1), (0,2)."""
    return None if C is None else dict(cameras=np.arange(C), pairs=[(2, 3), (3, 2), (2, C - 1), (0, 2)])


def sigma_reference(cams, pts, ci, pi, qs, fixed, loss=None, delta=1.0):
    """(Sigma [9C, 9C] by route (i), zeros on held rows and columns; the
    correlation-scaled spread between routes (i) and (ii); cond(S0))."""
    C, P = len(cams), len(pts)
    r, J = oba.residual_and_jacobian(cams, pts, ci, pi, qs)
    if loss is not None:  # sqrt(w), w = rho'(z), z = |r|^2 / delta^2 of the clamped residual
        z = np.sum(r * r, axis=1) / delta ** 2
        w = {"cauchy": 1.0 / (1.0 + z), "soft_l1": 1.0 / np.sqrt(1.0 + z),
             "huber": np.where(z > 1.0, 1.0 / np.sqrt(np.maximum(z, 1.0)), 1.0)}[loss]
        J = J * np.sqrt(w)[:, None, None]
    n = 9 * C + 3 * P
    Jd = np.zeros((2 * len(ci), n))
    rows = np.arange(len(ci))
    for q in range(2):
        Jd[(2 * rows + q)[:, None], (ci * 9)[:, None] + np.arange(9)] = J[:, q, :9]
        Jd[(2 * rows + q)[:, None], (9 * C + pi * 3)[:, None] + np.arange(3)] = J[:, q, 9:]
    free_c = np.nonzero(np.asarray(fixed).reshape(-1) == 0)[0]
    free = np.concatenate([free_c, 9 * C + np.arange(3 * P)])
    Jf = Jd[:, free]
    H = Jf.T @ Jf
    nc = len(free_c)
    s1 = np.linalg.inv(H)[:nc, :nc]  # route (i)
    U, W = H[:nc, :nc], H[:nc, nc:]
    V = H[nc:, nc:].reshape(P, 3, P, 3)[np.arange(P), :, np.arange(P), :]
    Y = np.einsum("cpi,pij->cpj", W.reshape(nc, P, 3), np.linalg.inv(V)).reshape(nc, 3 * P)
    S0 = U - Y @ W.T
    Li = np.linalg.inv(np.linalg.cholesky(0.5 * (S0 + S0.T)))
    s2 = Li.T @ Li  # route (ii)
    d = np.sqrt(np.diag(s1))
    spread = float(np.max(np.abs(s1 - s2) / np.outer(d, d)))
    full = np.zeros((9 * C, 9 * C))
    full[np.ix_(free_c, free_c)] = s1
    full.setflags(write=False)
    return full, spread, float(np.linalg.cond(S0))


def shape_reference(shape, intr_held):
    key = (shape, intr_held)
    if key not in _REFS:
        pr = problem(shape)
        _REFS[key] = sigma_reference(*pr, gauge(len(pr[0]), intr_held))
    return _REFS[key]


def blocks_of(full, pairs):
    return np.stack([full[9 * a:9 * a + 9, 9 * b:9 * b + 9] for a, b in pairs])


def deviation(got, full, pairs):
    """Largest correlation-scaled |got - reference| over the free entries of the blocks."""
    d = np.sqrt(np.diag(full))
    worst = 0.0
    for blk, (a, b) in zip(got, pairs):
        sc = np.outer(d[9 * a:9 * a + 9], d[9 * b:9 * b + 9])
        m = sc > 0
        if m.any():
            worst = max(worst, float(np.max(np.abs(blk - full[9 * a:9 * a + 9, 9 * b:9 * b + 9])[m] / sc[m])))
    return worst


def check_structure(got, pairs, fixed, C):
    """Held rows / columns exact zeros, marginal blocks exactly symmetric, (2,3) =
    (3,2)^T bitwise, (0,2) all zeros (camera 0 is held)."""
    assert got.shape == (len(pairs), 9, 9) and got.dtype == np.float64
    assert np.all(np.isfinite(got))
    idx = {tuple(p): i for i, p in enumerate(pairs.tolist())}
    for blk, (a, b) in zip(got, pairs):
        ha, hb = fixed[a] != 0, fixed[b] != 0
        assert np.all(blk[ha, :] == 0.0) and np.all(blk[:, hb] == 0.0)
        assert not np.any(np.signbit(blk[ha, :])) and not np.any(np.signbit(blk[:, hb]))
        if a == b:
            assert np.array_equal(blk, blk.T)
            assert np.all(np.diag(blk)[~ha] > 0.0)
    assert np.array_equal(got[idx[(2, 3)]].view(np.uint64), got[idx[(3, 2)]].T.copy().view(np.uint64))
    assert np.all(got[idx[(0, 2)]] == 0.0)


# ----------------------------------------------------------------------------- host
def test_cov_pairs_accepts():
    from slam355 import ba

    p = ba.cov_pairs(4)
    assert p.dtype == np.int32 and p.tolist() == [[0, 0], [1, 1], [2, 2], [3, 3]]
    assert ba.cov_pairs(4, cameras=[2, 0]).tolist() == [[2, 2], [0, 0]]
    assert ba.cov_pairs(4, pairs=[(1, 3), (3, 1), (2, 2)]).tolist() == [[1, 3], [3, 1], [2, 2]]
    assert ba.cov_pairs(4, cameras=np.array([3]), pairs=np.array([[0, 1]])).tolist() == [[3, 3], [0, 1]]
    assert ba.cov_pairs(4, cameras=[], pairs=[(0, 1)]).tolist() == [[0, 1]]
    assert ba.cov_pairs(1).tolist() == [[0, 0]]
    assert ba.cov_pairs(5, **request(5)).shape == (9, 2) and ba.cov_pairs(5, **request(5)).flags.c_contiguous


@pytest.mark.parametrize("kw", [dict(cameras=[4]), dict(cameras=[-1]), dict(pairs=[(0, 4)]), dict(pairs=[(-1, 0)]),
                                dict(pairs=[0, 1]), dict(pairs=[(0, 1, 2)]), dict(cameras=[[0, 1]]),
                                dict(cameras=[0.5]), dict(pairs=[(0.0, 1.0)]), dict(cameras=[True]),
                                dict(cameras=[]), dict(pairs=[]), dict(cameras=["a"])])
def test_cov_pairs_rejects(kw):
    from slam355 import ba

    with pytest.raises(ValueError):
        ba.cov_pairs(4, **kw)
    with pytest.raises(ValueError):
        ba.cov_pairs(0)


def test_signatures_hold_the_new_symbols():
    from slam355 import _lib

    assert len(_lib.SIGNATURES["slam_ba_cov_workspace_len"]) == 1
    assert len(_lib.SIGNATURES["slam_ba_covariance"]) == 9
    assert _lib.lib.slam_ba_cov_workspace_len.restype is ctypes.c_longlong
    assert _lib.lib.slam_abi_version() == 1
    # two dense matrices of T = ceil(9C / 64) tile rows, and a little more; 0 on bad sizes
    for C, T in ((6, 1), (10, 2), (15, 3), (30, 5), (64, 9), (500, 71)):
        n = _lib.lib.slam_ba_cov_workspace_len(C)
        assert 2 * (64 * T) ** 2 < n <= 2 * (64 * T) ** 2 + 64 * T + T * T + 16, (C, n)
    assert _lib.lib.slam_ba_cov_workspace_len(0) == 0 and _lib.lib.slam_ba_cov_workspace_len(-3) == 0


@pytest.mark.parametrize("intr_held", [False, True])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_reference_routes_agree(shape, intr_held):
    """The condition on the reference: its two routes agree to <= 1e-9
    (correlation-scaled) on every GPU-test problem."""
    full, spread, cond = shape_reference(shape, intr_held)
    print(f"{shape} intrinsics {'held' if intr_held else 'free'}: spread {spread:.2e}, cond(S0) {cond:.2e}")
    assert spread <= SPREAD_MAX
    fx = gauge(SHAPES[shape][0], intr_held).reshape(-1) != 0
    assert np.all(full[fx, :] == 0.0) and np.all(full[:, fx] == 0.0)
    assert np.all(np.diag(full)[~fx] > 0.0)


# ----------------------------------------------------------------------------- GPU
_CASES = [(s, h, "auto") for s in SHAPES for h in (False, True)] + \
         [(s, h, "slot") for s in ("6x150", "10x300") for h in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,intr_held,lin_mode", _CASES)
def test_gpu_covariance_matches_reference(shape, intr_held, lin_mode):
    from slam355 import ba

    pr = problem(shape)
    C = len(pr[0])
    fx = gauge(C, intr_held)
    full, spread, cond = shape_reference(shape, intr_held)
    assert spread <= SPREAD_MAX
    prob = ba.BAProblem(*pr, fixed=fx, lin_mode=lin_mode)
    assert prob.lin_mode == ("slot" if lin_mode == "slot" else "mfma")
    assert prob.tl_levels == (9 * C > 120)
    pairs = ba.cov_pairs(C, **request(C))
    got = prob.covariance(**request(C))
    dev = deviation(got, full, pairs)
    print(f"{shape} intrinsics {'held' if intr_held else 'free'} {prob.lin_mode}: deviation {dev:.2e}, "
          f"reference spread {spread:.2e} (bar {MARGIN * spread:.2e}), cond(S0) {cond:.2e}")
    check_structure(got, pairs, fx, C)
    assert dev <= MARGIN * spread
    assert prob.cov_status() == 0
    # a second call (workspace kept) and a sub-request give the same bits
    assert np.array_equal(prob.covariance(**request(C)), got)
    assert np.array_equal(prob.covariance(cameras=[2], pairs=[(2, C - 1)]), got[[2, len(pairs) - 2]])
    assert np.array_equal(prob.covariance(), got[:C])


@pytest.mark.gpu
def test_gpu_covariance_at_live_parameters():
    """After iterate(3) the blocks are those of the reference at exactly params()."""
    from slam355 import ba
    from slam355.synthetic import perturb

    cams, pts, ci, pi, qs = problem("15x400")
    C = len(cams)
    fx = gauge(C, False)
    prob = ba.BAProblem(*perturb(np.random.default_rng(5), cams, pts), ci, pi, qs, fixed=fx)
    prob.iterate(3)
    assert prob.state()["NACCEPT"] >= 1
    lc, lp = prob.params()
    assert not np.array_equal(lc, cams)
    full, spread, cond = sigma_reference(lc, lp, ci, pi, qs, fx)
    assert spread <= SPREAD_MAX
    pairs = ba.cov_pairs(C, **request(C))
    got = prob.covariance(**request(C))
    dev = deviation(got, full, pairs)
    print(f"live 15x400: deviation {dev:.2e}, spread {spread:.2e}, cond(S0) {cond:.2e}")
    check_structure(got, pairs, fx, C)
    assert dev <= MARGIN * spread


@pytest.mark.gpu
def test_gpu_covariance_robust():
    """loss = cauchy, f_scale 1.5, 10 % of the observations displaced by up to
    +-60 px: the blocks are those of the sqrt(w)-weighted Jacobian."""
    from slam355 import ba

    cams, pts, ci, pi, qs = problem("10x300")
    C = len(cams)
    rng = np.random.default_rng(11)
    out = rng.random(len(qs)) < 0.1
    qs = qs.copy()
    qs[out] += rng.uniform(-60, 60, (int(out.sum()), 2))
    fx = gauge(C, False)
    full, spread, cond = sigma_reference(cams, pts, ci, pi, qs, fx, "cauchy", 1.5)
    plain = sigma_reference(cams, pts, ci, pi, qs, fx)[0]
    assert spread <= SPREAD_MAX
    pairs = ba.cov_pairs(C, **request(C))
    assert deviation(blocks_of(plain, pairs), full, pairs) > 1e-2  # the weights matter here
    prob = ba.BAProblem(cams, pts, ci, pi, qs, fixed=fx, loss="cauchy", f_scale=1.5)
    got = prob.covariance(**request(C))
    dev = deviation(got, full, pairs)
    print(f"cauchy 10x300: deviation {dev:.2e}, spread {spread:.2e}, cond(S0) {cond:.2e}")
    check_structure(got, pairs, fx, C)
    assert dev <= MARGIN * spread


@pytest.mark.gpu
def test_gpu_covariance_scale():
    """scale="residual" = unit x 2 COST / (2 O - n_free); a float scale likewise; to 1e-15 relative."""
    import torch
    from slam355 import ba
    from slam355.synthetic import perturb

    cams, pts, ci, pi, qs = problem("10x300")
    C, P, O = len(cams), len(pts), len(qs)
    fx = gauge(C, True)
    prob = ba.BAProblem(*perturb(np.random.default_rng(5), cams, pts), ci, pi, qs, fixed=fx)
    prob.iterate(4)
    unit = prob.covariance()
    n_free = int((fx == 0).sum()) + 3 * P
    assert n_free == 9 * C + 3 * P - (18 + 3 * (C - 2))
    s2 = 2.0 * prob.state()["COST"] / (2 * O - n_free)
    assert s2 > 0.0
    for scale, fac in (("residual", s2), (2.5, 2.5), ("unit", 1.0)):
        got = prob.covariance(scale=scale)
        assert np.all(np.abs(got - unit * fac) <= 1e-15 * np.abs(unit * fac))
    dev = prob.covariance(scale="residual", device=True)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float64
    assert np.array_equal(dev.cpu().numpy(), prob.covariance(scale="residual"))
    for bad in ("sigma", 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            prob.covariance(scale=bad)
    for bad in (-1e-3, 1.0, float("nan")):
        with pytest.raises(ValueError):
            prob.covariance(rank_tol=bad)
    with pytest.raises(ValueError):
        prob.covariance(cameras=[C])


@pytest.mark.gpu
@pytest.mark.parametrize("graphed", [False, True])
@pytest.mark.parametrize("shape", ["6x150", "15x400"])
def test_gpu_covariance_has_no_side_effects(shape, graphed):
    """iterate(3); covariance(); iterate(3) equals iterate(6) on a twin: the
    parameters and the LM state slots bit for bit."""
    from slam355 import ba
    from slam355.synthetic import perturb

    cams, pts, ci, pi, qs = problem(shape)
    fx = gauge(len(cams), False)
    start = perturb(np.random.default_rng(5), cams, pts)
    a = ba.BAProblem(*start, ci, pi, qs, fixed=fx)
    b = ba.BAProblem(*start, ci, pi, qs, fixed=fx)
    step = (lambda p, n: p.iterate_graphed(n)) if graphed else (lambda p, n: p.iterate(n))
    step(a, 3)
    before = a.state()
    a.covariance(**request(len(cams)))
    after = a.state()
    assert all(np.float64(before[k]).tobytes() == np.float64(after[k]).tobytes() for k in before)
    step(a, 3)
    step(b, 6)
    sa, sb = a.state(), b.state()
    assert sa["NACCEPT"] >= 2
    for k in ST_SLOTS:
        assert np.float64(sa[k]).tobytes() == np.float64(sb[k]).tobytes(), k
    for x, y in zip(a.params(), b.params()):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("anchors", [1, 0])
def test_gpu_covariance_reports_rank_deficiency(anchors):
    """Only camera 0 held, or nothing held: the gauge is free, a relative
    pivot falls under rank_tol, LinAlgError; device=True gives NaN blocks and
    status 1."""
    import torch
    from slam355 import ba

    pr = problem("10x300")
    C = len(pr[0])
    prob = ba.BAProblem(*pr, fixed=gauge(C, False, anchors) if anchors else None)
    with pytest.raises(np.linalg.LinAlgError):
        prob.covariance()
    out = prob.covariance(**request(C), device=True)
    torch.cuda.synchronize()
    assert prob.cov_status() == 1
    assert out.shape == (C + 4, 9, 9) and bool(torch.isnan(out).all())
    # the same problem with the gauge fixed by the mask is fine afterwards (status cleared)
    ok = ba.BAProblem(*pr, fixed=gauge(C, False))
    assert np.all(np.isfinite(ok.covariance())) and ok.cov_status() == 0


@pytest.mark.gpu
def test_gpu_window_set_covariance_equals_problem():
    """A BAWindowSet.build window's covariance() is the one of the same problem
    built as a BAProblem, bit for bit; after the set reused its buffers it raises."""
    import torch
    from slam355 import ba

    pr = problem("10x300")
    C = len(pr[0])
    fx = gauge(C, True)
    s = torch.cuda.Stream()
    ws = ba.BAWindowSet()
    win = ws.build([pr, problem("6x150")], s, fixed=ba.FIXED_INTRINSICS)[0]
    win = ws.build([pr], s, fixed=fx)[0]
    assert type(win).__name__ == "_WindowProblem"
    ref = ba.BAProblem(*pr, fixed=fx)
    for p in (win, ref):
        p.iterate(2)
    got = win.covariance(**request(C))
    exp = ref.covariance(**request(C))
    assert np.array_equal(got.view(np.uint64), exp.view(np.uint64))
    ws.build([pr], s, fixed=fx)
    ws.build([pr], s, fixed=fx)
    with pytest.raises(RuntimeError):
        win.covariance()


@pytest.mark.gpu
def test_gpu_batch_covariance_equals_per_problem_calls():
    from slam355 import ba

    specs = [("6x150", False), ("10x300", True), ("6x150", True)]
    probs = [ba.BAProblem(*problem(s), fixed=gauge(SHAPES[s][0], h)) for s, h in specs]
    batch = ba.BABatch(probs)
    batch.iterate(2)
    got = batch.covariance(cameras=[2, 3], pairs=[(2, 5)], scale=2.0)
    assert isinstance(got, list) and len(got) == 3
    for g, p in zip(got, probs):
        assert g.shape == (3, 9, 9)
        assert np.array_equal(g, p.covariance(cameras=[2, 3], pairs=[(2, 5)], scale=2.0))


@pytest.mark.gpu
def test_gpu_c_abi_refusals():
    """A short or null workspace, n_pairs = 0 and rank_tol = nan return non-zero
    with a message and launch nothing (the status word keeps its sentinel)."""
    import torch
    from slam355 import _lib, ba

    pr = problem("6x150")
    prob = ba.BAProblem(*pr, fixed=gauge(6, False))
    prob.iterate(1)
    lam = prob.state()["LAMBDA"]
    n = int(_lib.lib.slam_ba_cov_workspace_len(6))
    ws = torch.zeros(n, dtype=torch.float64, device="cuda")
    pairs = torch.from_numpy(ba.cov_pairs(6)).cuda()
    out = torch.full((6, 9, 9), 5.0, dtype=torch.float64, device="cuda")
    status = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    sp = ba.stream_ptr()

    def call(n_pairs, tol, wsp, ws_len):
        return _lib.lib.slam_ba_covariance(ctypes.byref(prob._s), pairs.data_ptr(), n_pairs, tol,
                                           out.data_ptr(), wsp, ws_len, status.data_ptr(), sp)

    for args, word in (((6, 1e-8, ws.data_ptr(), n - 1), b"workspace"), ((6, 1e-8, None, n), b"workspace"),
                       ((0, 1e-8, ws.data_ptr(), n), b"n_pairs"), ((-2, 1e-8, ws.data_ptr(), n), b"n_pairs"),
                       ((6, float("nan"), ws.data_ptr(), n), b"rank_tol"),
                       ((6, float("inf"), ws.data_ptr(), n), b"rank_tol"),
                       ((6, 1.0, ws.data_ptr(), n), b"rank_tol"), ((6, -1e-9, ws.data_ptr(), n), b"rank_tol")):
        assert call(*args) != 0, args
        assert word in _lib.lib.slam_last_error(), (args, _lib.lib.slam_last_error())
    torch.cuda.synchronize()
    assert int(status.item()) == 7 and bool((out == 5.0).all())
    assert prob.state()["LAMBDA"] == lam
    assert call(6, 1e-8, ws.data_ptr(), n) == 0  # and the accepted call runs
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert np.array_equal(out.cpu().numpy(), prob.covariance())
    assert prob.state()["LAMBDA"] == lam
