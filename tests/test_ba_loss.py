"""Bundle adjustment with a robust loss per observation (slam_ba_problem.loss /
loss_scale, slam355.ba.loss_args / BAProblem(loss=, f_scale=)).

Semantics: with r the clamped 2-vector residual of an
observation, J its 2 x 12 Jacobian (held columns removed), s = |r|^2,
d = f_scale and z = s / d^2, the observation enters the LM iteration as
sqrt(w) r, sqrt(w) J with w = rho'(z) (Gauss-Newton / IRLS, no rho'' term), and
the LM cost is 0.5 d^2 sum rho(z) at the live and at the trial parameters;
rho is scipy's (linear z; huber z | 2 sqrt(z) - 1; soft_l1 2 (sqrt(1 + z) - 1);
cauchy log(1 + z)).  Everything else is oracle.ba.lm_iteration /
lm_iteration_schur.

Reference: this file's NumPy restatement of those two oracle iterations on
(r~, J~) with the two cost substitutions (_lm_dense, _lm_schur).

Inputs: ba_problem(default_rng(3), C, P, 4, f=716.8, noise=0.5), the
perturbation of tests/test_ba_fixed.py from default_rng(pseed), 10 % of the
observations displaced by up to +-60 px, and three gross outliers (+8000 px on
x twice, -9000 px on y once) so that the reference's 5000 px clamp is active
under the loss.  d = 1.5 px, lambda0 = 1e-4.

Bars (float64), those of tests/test_ba_fixed.py: accept flag equal, COST_NEW
1e-9 relative (tiled solve: 1e-8), lambda 1e-6 relative, cameras and points
rtol 1e-6 / atol 1e-9, CHOL_FAIL 0.  Precondition (a condition on the
reference, not a tolerance): in every compared iteration the reference's
|rho| >= 0.05, so no accept flag is decided by rounding.
"""
import ctypes
import os
import socket

import numpy as np
import pytest

from oracle import ba as oba
from stage_ref import stage_inputs

DELTA = 1.5
LAM0 = 1e-4
LOSS_NAMES = ("linear", "huber", "soft_l1", "cauchy")


# ----------------------------------------------------------------------------- inputs
def make_problem(seed, C, P, obs_per_pt):
    from slam355.synthetic import ba_problem

    return ba_problem(np.random.default_rng(seed), C, P, obs_per_pt, f=716.8, noise=0.5)


def _perturb(rng, cams, pts):
    """The perturbation of tests/test_ba_fixed.py."""
    C = len(cams)
    cams0 = cams.copy()
    cams0[:, :3] += rng.normal(0, 1e-3, (C, 3))
    cams0[:, 3:6] += rng.normal(0, 1e-2, (C, 3))
    return cams0, pts + rng.normal(0, 0.05, pts.shape)


_CASES = {}


def outlier_case(C, P, pseed):
    """(c0, p0, ci, pi, qs), shared by the tests and never written: the start
    and the observations with their outliers (module docstring)."""
    key = (C, P, pseed)
    if key not in _CASES:
        cams, pts, ci, pi, qs = make_problem(3, C, P, 4)
        rng = np.random.default_rng(pseed)
        c0, p0 = _perturb(rng, cams, pts)
        O = len(qs)
        out = rng.random(O) < 0.1
        qs = qs.copy()
        qs[out] += rng.uniform(-60, 60, (int(out.sum()), 2))
        gi = np.random.default_rng(100 + pseed).choice(O, 3, replace=False)
        qs[gi[:2], 0] += 8000.0
        qs[gi[2], 1] -= 9000.0
        _CASES[key] = (c0, p0, ci, pi, qs)
    return _CASES[key]


def _held(words):
    return ((np.asarray(words)[:, None] >> np.arange(9, dtype=np.uint32)) & 1).astype(bool)


def _fixed_small():
    """The `fixed` pattern of test_ba_fixed._case_small."""
    from slam355 import ba

    fixed = np.tile(ba.FIXED_INTRINSICS, (6, 1))
    fixed[0] = 1
    fixed[1, 5] = 1
    return fixed


# ----------------------------------------------------------------------------- reference
def rho_w(z, loss):
    """rho(z) and w = rho'(z) of scipy's least_squares losses."""
    z = np.asarray(z, np.float64)
    if loss == "linear":
        return z.copy(), np.ones_like(z)
    if loss == "huber":
        big = z > 1.0
        sq = np.sqrt(np.where(big, z, 1.0))
        return np.where(big, 2.0 * sq - 1.0, z), np.where(big, 1.0 / sq, 1.0)
    if loss == "soft_l1":
        sq = np.sqrt(1.0 + z)
        return 2.0 * (sq - 1.0), 1.0 / sq
    if loss == "cauchy":
        return np.log1p(z), 1.0 / (1.0 + z)
    raise ValueError(loss)


def robust_rj(cams, pts, ci, pi, qs, loss, delta, words=None):
    """(r~, J~, cost terms d^2 rho(z) per observation) from the oracle's
    clamped residual and Jacobian; words: held-parameter mask words."""
    r, J = oba.residual_and_jacobian(cams, pts, ci, pi, qs)
    if words is not None:
        J = J.copy()
        held = _held(words)[np.asarray(ci)]
        J[:, :, :9][np.broadcast_to(held[:, None, :], J[:, :, :9].shape)] = 0.0
    if loss == "linear":  # d^2 rho(z) = s exactly; nothing is scaled
        return r, J, np.sum(r * r, axis=1)
    z = np.sum(r * r, axis=1) / delta ** 2
    rho, w = rho_w(z, loss)
    sw = np.sqrt(w)
    return r * sw[:, None], J * sw[:, None, None], delta ** 2 * rho


def robust_cost(cams, pts, ci, pi, qs, loss, delta):
    return 0.5 * float(np.sum(robust_rj(cams, pts, ci, pi, qs, loss, delta)[2]))


def _accept(st, rho, accepted):
    if accepted:
        st.lam = min(max(st.lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), oba.LAM_MIN), oba.LAM_MAX)
        st.nu = 2.0
    else:
        st.lam = min(st.lam * st.nu, oba.LAM_MAX)
        st.nu *= 2.0


def _lm_dense(cams, pts, ci, pi, qs, st, loss, delta, words=None):
    """oracle.ba.lm_iteration on (r~, J~); cost and cost_new are the robust ones
    (for "linear" the oracle's own expressions, so it is reproduced exactly)."""
    C, P = len(cams), len(pts)
    r, J, terms = robust_rj(cams, pts, ci, pi, qs, loss, delta, words)
    n = 9 * C + 3 * P
    Jd = np.zeros((2 * len(ci), n))
    rows = np.arange(len(ci))
    for q in range(2):
        Jd[(2 * rows + q)[:, None], (ci * 9)[:, None] + np.arange(9)] = J[:, q, :9]
        Jd[(2 * rows + q)[:, None], (9 * C + pi * 3)[:, None] + np.arange(3)] = J[:, q, 9:]
    rv = r.ravel()
    H, g = Jd.T @ Jd, -Jd.T @ rv
    cost = 0.5 * float(rv @ rv) if loss == "linear" else 0.5 * float(np.sum(terms))
    D = np.clip(np.diag(H), oba.DIAG_MIN, oba.DIAG_MAX)
    delta_x = np.linalg.solve(H + st.lam * np.diag(D), g)
    cams_n = cams + delta_x[: 9 * C].reshape(C, 9)
    pts_n = pts + delta_x[9 * C:].reshape(-1, 3)
    if loss == "linear":
        rn = oba.residual_and_jacobian(cams_n, pts_n, ci, pi, qs)[0]
        cost_new = 0.5 * float(np.sum(rn * rn))
    else:
        cost_new = robust_cost(cams_n, pts_n, ci, pi, qs, loss, delta)
    pred = 0.5 * float(delta_x @ (st.lam * D * delta_x + g))
    rho = (cost - cost_new) / pred if pred > 0 else -1.0
    accepted = rho > 0
    _accept(st, rho, accepted)
    if accepted:
        cams, pts = cams_n, pts_n
    return cams, pts, dict(cost=cost, cost_new=cost_new, pred=pred, rho=rho, accepted=accepted, g=g)


def _lm_schur(cams, pts, ci, pi, qs, st, loss, delta, pairs, words=None):
    """oracle.ba.lm_iteration_schur on (r~, J~) with the robust costs."""
    C, P = len(cams), len(pts)
    r, J, terms = robust_rj(cams, pts, ci, pi, qs, loss, delta, words)
    cost = 0.5 * float(np.sum(terms))
    Jc, Jp = J[:, :, :9], J[:, :, 9:]
    U = np.zeros((C, 9, 9))
    np.add.at(U, ci, np.einsum("oai,oaj->oij", Jc, Jc))
    V = np.zeros((P, 3, 3))
    np.add.at(V, pi, np.einsum("oai,oaj->oij", Jp, Jp))
    gc = np.zeros((C, 9))
    np.add.at(gc, ci, -np.einsum("oai,oa->oi", Jc, r))
    gp = np.zeros((P, 3))
    np.add.at(gp, pi, -np.einsum("oai,oa->oi", Jp, r))
    Dc = np.clip(np.diagonal(U, axis1=1, axis2=2), oba.DIAG_MIN, oba.DIAG_MAX)
    Dp = np.clip(np.diagonal(V, axis1=1, axis2=2), oba.DIAG_MIN, oba.DIAG_MAX)
    Vi = np.linalg.inv(V + st.lam * Dp[:, :, None] * np.eye(3)[None])
    W = np.einsum("oai,oaj->oij", Jc, Jp)
    Y = np.einsum("oij,ojk->oik", W, Vi[pi])
    e = np.einsum("pij,pj->pi", Vi, gp)
    o1, o2 = pairs
    S = np.zeros((C, C, 9, 9))
    np.add.at(S, (ci[o1], ci[o2]), -np.einsum("oik,ojk->oij", Y[o1], W[o2]))
    S = S + np.transpose(S, (1, 0, 3, 2)) * (1 - np.eye(C))[:, :, None, None]
    S[np.arange(C), np.arange(C)] += U + st.lam * Dc[:, :, None] * np.eye(9)[None]
    b = gc.copy()
    np.add.at(b, ci, -np.einsum("oij,oj->oi", Y, gp[pi]))
    dc = np.linalg.solve(S.transpose(0, 2, 1, 3).reshape(9 * C, 9 * C), b.ravel()).reshape(C, 9)
    dp = e.copy()
    np.add.at(dp, pi, -np.einsum("oji,oj->oi", Y, dc[ci]))
    cams_n, pts_n = cams + dc, pts + dp
    cost_new = robust_cost(cams_n, pts_n, ci, pi, qs, loss, delta)
    pred = 0.5 * (float(np.sum(dc * (st.lam * Dc * dc + gc))) + float(np.sum(dp * (st.lam * Dp * dp + gp))))
    rho = (cost - cost_new) / pred if pred > 0 else -1.0
    accepted = rho > 0 and np.isfinite(cost_new)
    _accept(st, rho, accepted)
    if accepted:
        cams, pts = cams_n, pts_n
    return cams, pts, dict(cost=cost, cost_new=cost_new, pred=pred, rho=rho, accepted=accepted)


_REF = {}


def reference(C, P, pseed, loss, iters, schur, fixed=None):
    """The reference's iterates of one case, computed once and shared
    (read-only): (case, mask words or None, [(accepted, cost_new, lambda, cams,
    pts, rho)])."""
    key = (C, P, pseed, loss, iters, schur, fixed is not None)
    if key in _REF:
        return _REF[key]
    from slam355 import ba

    case = outlier_case(C, P, pseed)
    c0, p0, ci, pi, qs = case
    words = None if fixed is None else ba.fixed_mask(C, fixed)
    st = oba.LMState(LAM0)
    oc, op = c0.copy(), p0.copy()
    pairs = oba._obs_pairs(ci, pi) if schur else None
    recs = []
    for _ in range(iters):
        if schur:
            oc, op, info = _lm_schur(oc, op, ci, pi, qs, st, loss, DELTA, pairs, words)
        else:
            oc, op, info = _lm_dense(oc, op, ci, pi, qs, st, loss, DELTA, words)
        # precondition: the accept decision is not a matter of rounding
        assert abs(info["rho"]) >= 0.05, (key, info["rho"])
        recs.append((bool(info["accepted"]), info["cost_new"], st.lam, oc.copy(), op.copy(), info["rho"]))
    for rec in recs:
        rec[3].setflags(write=False)
        rec[4].setflags(write=False)
    _REF[key] = (case, words, recs)
    return _REF[key]


def _compare(prob, ref, cost_rtol):
    (c0, _, _, _, _), words, recs = ref
    for it, (acc, cost_new, lam, oc, op, rho) in enumerate(recs):
        prob.iterate(1)
        s = prob.state()
        gc, gp = prob.params()
        print(f"it {it}: accepted {s['ACCEPTED']:.0f}/{acc} (ref rho {rho:.3f}) cost_new {s['COST_NEW']:.9g} rel "
              f"{abs(s['COST_NEW'] - cost_new) / cost_new:.2e} lambda rel {abs(s['LAMBDA'] - lam) / lam:.2e} "
              f"cams {np.abs(gc - oc).max():.2e} pts {np.abs(gp - op).max():.2e}")
        assert s["CHOL_FAIL"] == 0.0, it
        assert bool(s["ACCEPTED"]) == acc, it
        assert abs(s["COST_NEW"] - cost_new) <= cost_rtol * cost_new + 1e-12, it
        assert abs(s["LAMBDA"] - lam) <= 1e-6 * lam, it
        assert np.allclose(gc, oc, rtol=1e-6, atol=1e-9), it
        assert np.allclose(gp, op, rtol=1e-6, atol=1e-9), it
        if words is not None:  # held entries: the input's bits, in both parameter buffers
            h = _held(words)
            for k in ("cams0", "cams1"):
                assert np.array_equal(prob.t[k].cpu().numpy()[h], c0[h]), (it, k)


# pseed of each 6 x 150 loss case (reference rho of the six dense iterations:
# huber 1.13 0.71 0.37 0.20 0.93 -0.33, cauchy 1.75 1.15 0.95 -0.22 0.79 0.73,
# soft_l1 1.28 1.20 0.91 -0.27 0.64 1.01), and of 14 x 400 huber (1.36 1.18 0.48 -0.41 0.65)
SMALL_PSEED = {"huber": 4, "cauchy": 1, "soft_l1": 1}
TILED_PSEED = 2
# huber with the held pattern of test_ba_fixed._case_small: the pseed in 1..8 chosen here
# because the masked reference meets the |rho| >= 0.05 precondition in all six iterations
FIXED_PSEED = 4


# ----------------------------------------------------------------------------- host
def test_loss_args():
    from slam355 import ba

    assert ba.LOSSES == {"linear": 0, "huber": 1, "soft_l1": 2, "cauchy": 3}
    for name, code in ba.LOSSES.items():
        assert ba.loss_args(name, 1.5) == (code, 1.5)
    assert ba.loss_args(None, 2.0) == (0, 2.0)
    assert ba.loss_args(None) == (0, 1.0) and ba.loss_args("linear") == (0, 1.0)
    assert isinstance(ba.loss_args("huber", 2)[1], float)


@pytest.mark.parametrize("loss,f_scale", [("l2", 1.0), ("Huber", 1.0), (1, 1.0), ("huber", 0), ("huber", -1),
                                          ("huber", float("nan")), ("cauchy", float("inf")),
                                          (None, 0.0), ("linear", float("nan")), ("huber", "x")])
def test_loss_args_rejects(loss, f_scale):
    from slam355 import ba

    with pytest.raises(ValueError):
        ba.loss_args(loss, f_scale)


def test_struct_layout():
    """loss at the old asm_pad offset (after n_asm_act), loss_scale immediately
    before cam_fixed, which stays last; 408 bytes on both sides."""
    from slam355 import _lib

    S = _lib.BAProblemStruct
    names = [f[0] for f in S._fields_]
    assert "asm_pad" not in names
    assert names[-3:] == ["loss", "loss_scale", "cam_fixed"]
    assert S.loss.offset == S.n_asm_act.offset + 4 == 388 and S.loss.size == 4
    assert S.loss_scale.offset == 392 and S.loss_scale.size == 8
    assert S.cam_fixed.offset == S.loss_scale.offset + 8 == ctypes.sizeof(S) - 8
    assert ctypes.sizeof(S) == _lib.lib.slam_ba_problem_size() == 408
    z = S()  # a zeroed descriptor is the plain loss
    assert z.loss == 0 and z.loss_scale == 0.0 and z.cam_fixed is None


@pytest.mark.parametrize("loss,scale,word", [(7, 1.5, "loss 7"), (-1, 1.5, "loss -1"), (1, 0.0, "loss_scale"),
                                             (3, -2.0, "loss_scale"), (2, float("nan"), "loss_scale"),
                                             (1, float("inf"), "loss_scale")])
def test_launchers_refuse_bad_loss_descriptor(loss, scale, word):
    """Every launcher checks the descriptor before it touches the device: a
    loss outside 0..3, or a robust loss without a finite positive scale, is an
    error status with a slam_last_error() text (single, batched, phases,
    distributed -- whose communicator is never reached)."""
    from slam355 import _lib

    arr = (_lib.BAProblemStruct * 2)()
    arr[0].n_cams = arr[1].n_cams = 6
    arr[1].loss, arr[1].loss_scale = loss, scale
    L = _lib.lib
    p = ctypes.byref(arr[1])
    calls = [lambda: L.slam_ba_iterate(p, 1, None), lambda: L.slam_ba_iterate_batch(p, 1, 1, None),
             lambda: L.slam_ba_reset(p, 1e-4, None), lambda: L.slam_ba_build_system(p, None),
             lambda: L.slam_ba_solve_step(p, None), lambda: L.slam_ba_decide(p, None),
             lambda: L.slam_ba_step_distributed(p, ctypes.c_void_p(8), None)]
    for fn in calls:
        assert fn() != 0
        msg = L.slam_last_error().decode()
        assert "slam_ba" in msg and word in msg, msg
    # a zeroed loss passes this check: the error is the next one (no buffers)
    assert L.slam_ba_iterate(ctypes.byref(arr[0]), 1, None) != 0
    assert "loss" not in L.slam_last_error().decode()


def test_reference_linear_is_the_oracle():
    """_lm_dense with "linear" reproduces oracle.ba.lm_iteration exactly."""
    c0, p0, ci, pi, qs = outlier_case(6, 150, 4)
    sa, sb = oba.LMState(LAM0), oba.LMState(LAM0)
    ca, pa, cb, pb = c0.copy(), p0.copy(), c0.copy(), p0.copy()
    for _ in range(3):
        ca, pa, ia = oba.lm_iteration(ca, pa, ci, pi, qs, sa)
        cb, pb, ib = _lm_dense(cb, pb, ci, pi, qs, sb, "linear", DELTA)
        assert all(ia[k] == ib[k] for k in ("cost", "cost_new", "pred", "rho", "accepted"))
        assert np.array_equal(ca, cb) and np.array_equal(pa, pb)
        assert sa.lam == sb.lam and sa.nu == sb.nu


def test_reference_rho_and_weights():
    """rho(0) = 0, rho'(0) = 1 (scipy's normalisation), w = d rho / dz, and
    huber's two branches meet at z = 1."""
    z = np.array([0.0, 1e-3, 0.5, 1.0, 1.0 + 1e-9, 4.0, 1e6])
    for loss in LOSS_NAMES:
        rho, w = rho_w(z, loss)
        assert rho[0] == 0.0 and w[0] == 1.0
        h = 1e-6 * np.maximum(z[1:], 1.0)
        num = (rho_w(z[1:] + h, loss)[0] - rho_w(z[1:] - h, loss)[0]) / (2 * h)
        if loss == "huber":  # rho'' jumps at z = 1: skip the two points at the kink
            keep = np.abs(z[1:] - 1.0) > 1e-3
            num, wz = num[keep], w[1:][keep]
        else:
            wz = w[1:]
        assert np.allclose(num, wz, rtol=1e-6)
    assert rho_w(np.array([1.0]), "huber")[0][0] == 1.0 and rho_w(np.array([4.0]), "huber")[0][0] == 3.0


@pytest.mark.parametrize("loss", LOSS_NAMES)
def test_reference_gradient_is_the_gradient_of_the_robust_cost(loss):
    """g = -J~^T r~ of the reference is minus the gradient of F = 0.5 d^2 sum
    rho(z): central differences of F over 20 random parameters.  The step and
    the bar come from the reference alone: h = 1e-6 max(1, |x|); the bar of an
    entry is the change of the difference quotient from step 2h to h (its
    truncation error is a third of that) plus the rounding of F in the
    quotient, 64 eps F / h (F is a sum of ~600 positive terms evaluated twice:
    a few eps F each).  This pins the semantics -- weights, per-observation z,
    the clamp's chain rule under the loss -- independently of the GPU."""
    c0, p0, ci, pi, qs = outlier_case(6, 150, 4)
    C = len(c0)
    g = _lm_dense(c0.copy(), p0.copy(), ci, pi, qs, oba.LMState(LAM0), loss, DELTA)[2]["g"]
    x0 = np.concatenate([c0.ravel(), p0.ravel()])

    def F(x):
        return robust_cost(x[:9 * C].reshape(C, 9), x[9 * C:].reshape(-1, 3), ci, pi, qs, loss, DELTA)

    F0 = F(x0)
    idx = np.random.default_rng(7).choice(len(x0), 20, replace=False)
    idx[:4] = [0, 5, 6, 8]  # a rotation, a translation, f and k2 among them
    eps = np.finfo(np.float64).eps
    for i in idx:
        h = 1e-6 * max(1.0, abs(x0[i]))
        q = []
        for step in (h, 2 * h):
            xp, xm = x0.copy(), x0.copy()
            xp[i] += step
            xm[i] -= step
            q.append((F(xp) - F(xm)) / (2 * step))
        bar = abs(q[1] - q[0]) + 64 * eps * F0 / h
        print(f"{loss} param {i}: -g {-g[i]:.9g} central difference {q[0]:.9g} diff {abs(q[0] + g[i]):.2e} bar {bar:.2e}")
        assert abs(q[0] + g[i]) <= bar, (loss, i)
        assert bar <= 1e-6 * np.abs(g).max()  # the check has teeth: far below the gradient's scale


def test_pose_chain_form_refuses_loss():
    from slam355 import BundleAdjustment as B

    with pytest.raises(ValueError):
        B.bundle_adjustment_with_sparsity(np.zeros(60), None, loss="huber")
    with pytest.raises(ValueError):
        B.bundle_adjustment_with_sparsity(np.zeros(60), None, f_scale=2.0)


# ----------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("lin_mode", ["auto", "slot"])
@pytest.mark.parametrize("loss", ["huber", "soft_l1", "cauchy"])
def test_gpu_loss_small_matches_reference(loss, lin_mode):
    """6 x 150, one-workgroup solve, both linearisations (k_lin_mfma under
    "auto", k_linearize under "slot"): 6 LM iterates equal the dense
    reference; both huber branches, the clamp and a rejected step occur."""
    from slam355 import ba

    ref = reference(6, 150, SMALL_PSEED[loss], loss, 6, schur=False)
    c0, p0, ci, pi, qs = ref[0]
    assert not all(r[0] for r in ref[2])  # a rejected step is among the compared ones
    prob = ba.BAProblem(c0, p0, ci, pi, qs, lam0=LAM0, lin_mode=lin_mode, loss=loss, f_scale=DELTA)
    assert prob.lin_mode == ("slot" if lin_mode == "slot" else "mfma")
    assert prob.loss == loss and prob.f_scale == DELTA
    assert prob._s.loss == ba.LOSSES[loss] and prob._s.loss_scale == DELTA
    _compare(prob, ref, 1e-9)
    # residuals() stays raw: the clamped, unweighted residual at the solution
    gc, gp = prob.params()
    assert np.allclose(ba.residuals(gc, gp, ci, pi, qs), oba.residual_and_jacobian(gc, gp, ci, pi, qs)[0],
                       rtol=1e-9, atol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["flow", "levels", "fold"])
def test_gpu_loss_tiled_solve_matches_reference(how):
    """14 x 400 huber (9C = 126 > 120): the tiled camera solve, dataflow and
    level-scheduled, 5 iterates against the Schur reference; and the same
    problem with the assembly folded into k_lin_mfma.  The folded and the
    separate assembly sum their partial rows in different orders (rows_sum in
    csrc/ba.hip: "each form gives its own bits"), so they are not bit-equal
    with or without a loss: the folded form is held to the same bars."""
    from slam355 import ba

    ref = reference(14, 400, TILED_PSEED, "huber", 5, schur=True)
    c0, p0, ci, pi, qs = ref[0]
    kw = dict(fold_assembly=True) if how == "fold" else dict(tl_mode=how)
    prob = ba.BAProblem(c0, p0, ci, pi, qs, lam0=LAM0, loss="huber", f_scale=DELTA, **kw)
    assert prob.tl_levels and prob.lin_mode == "mfma"
    assert (prob._s.asm_tab is not None) == (how == "fold")
    _compare(prob, ref, 1e-8)


@pytest.mark.gpu
@pytest.mark.parametrize("lin_mode", ["auto", "slot"])
def test_gpu_loss_with_held_parameters_matches_reference(lin_mode):
    """Huber and the held pattern of test_ba_fixed._case_small together: the
    reference with both the mask and the loss; held entries keep the input's
    bits."""
    from slam355 import ba

    fixed = _fixed_small()
    ref = reference(6, 150, FIXED_PSEED, "huber", 6, schur=False, fixed=fixed)
    c0, p0, ci, pi, qs = ref[0]
    prob = ba.BAProblem(c0, p0, ci, pi, qs, lam0=LAM0, lin_mode=lin_mode, fixed=fixed, loss="huber",
                        f_scale=DELTA)
    _compare(prob, ref, 1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("lin_mode", ["auto", "slot"])
def test_gpu_linear_keyword_is_the_default_path(lin_mode):
    """loss="linear" (any f_scale) and no keyword: equal parameters and equal
    state slots, all of them, after each of 6 iterations."""
    from slam355 import ba

    c0, p0, ci, pi, qs = outlier_case(6, 150, 4)
    a = ba.BAProblem(c0, p0, ci, pi, qs, lin_mode=lin_mode)
    b = ba.BAProblem(c0, p0, ci, pi, qs, lin_mode=lin_mode, loss="linear", f_scale=3.0)
    assert a.loss == b.loss == "linear" and a._s.loss == b._s.loss == 0
    for it in range(6):
        a.iterate(1)
        b.iterate(1)
        assert np.array_equal(a.t["state"].cpu().numpy(), b.t["state"].cpu().numpy()), it
        for k in ("cams0", "cams1", "pts0", "pts1"):
            assert np.array_equal(a.t[k].cpu().numpy(), b.t[k].cpu().numpy()), (it, k)
    assert a.state()["NACCEPT"] >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("lin_mode", ["auto", "slot"])
def test_gpu_huber_with_a_huge_scale_is_the_plain_step(lin_mode):
    """Huber with f_scale = 1e9: every z <= 1, every weight 1, so the first
    trial parameters are the plain problem's bit for bit and the trial cost
    agrees (1e-12 relative)."""
    from slam355 import ba

    c0, p0, ci, pi, qs = outlier_case(6, 150, 4)
    a = ba.BAProblem(c0, p0, ci, pi, qs, lin_mode=lin_mode)
    b = ba.BAProblem(c0, p0, ci, pi, qs, lin_mode=lin_mode, loss="huber", f_scale=1e9)
    a.iterate(1)
    b.iterate(1)
    for k in ("cams1", "pts1"):  # the first trial goes to buffer 1
        assert np.array_equal(a.t[k].cpu().numpy(), b.t[k].cpu().numpy()), k
    sa, sb = a.state(), b.state()
    print(f"COST_NEW plain {sa['COST_NEW']!r} huber(1e9) {sb['COST_NEW']!r} COST {sa['COST']!r} {sb['COST']!r}")
    assert abs(sa["COST_NEW"] - sb["COST_NEW"]) <= 1e-12 * sa["COST_NEW"]


def _three_windows():
    return [(outlier_case(6, 150, 4), None), (outlier_case(6, 150, 4), "huber"), (outlier_case(6, 150, 1), "cauchy")]


@pytest.mark.gpu
def test_gpu_losses_in_one_batch_equal_solo():
    """A BABatch of three 6 x 150 windows with linear, huber and cauchy (one
    launch set, a loss per grid row) equals the three problems iterated
    alone, bit for bit, after 4 iterations."""
    from slam355 import ba

    mk = lambda: [ba.BAProblem(*w, loss=ls, f_scale=DELTA) for w, ls in _three_windows()]  # noqa: E731
    solo = mk()
    for p in solo:
        p.iterate(4)
    batch = ba.BABatch(mk())
    batch.iterate(4)
    for a, b in zip(solo, batch.problems):
        assert a.state() == b.state()
        for x, y in zip(a.params(), b.params()):
            assert np.array_equal(x, y)
    assert solo[0].state()["COST"] != solo[1].state()["COST"]  # the loss did something


@pytest.mark.gpu
def test_gpu_window_set_loss_equals_separate_problems():
    """BAWindowSet.build(loss="huber", f_scale=1.5) gives every window the
    iterates BAProblem(loss="huber") gives it alone, bit for bit; a later call
    without the keyword is plain again."""
    import torch
    from slam355 import ba

    wins = [outlier_case(6, 150, 4), outlier_case(6, 150, 1), outlier_case(6, 150, 2)]
    s = torch.cuda.Stream()
    ws = ba.BAWindowSet()
    for kw in (dict(loss="huber", f_scale=DELTA), dict()):
        got = ws.build(wins, s, **kw)
        assert all(p.loss == kw.get("loss", "linear") and p._s.loss == ba.LOSSES[p.loss] for p in got)
        with torch.cuda.stream(s):
            ba.BABatch(got, stream=s).iterate(4)
        torch.cuda.synchronize()
        for w, p in zip(wins, got):
            ref = ba.BAProblem(*w, **kw)
            ref.iterate(4)
            assert ref.state() == p.state()
            for x, y in zip(ref.params(), p.params()):
                assert np.array_equal(x, y)


@pytest.mark.gpu
def test_gpu_window_set_stage_loss_equals_separate_problems():
    """BAWindowSet.stage(loss="cauchy"): the natively staged descriptors (which
    the native call zeroes: plain loss) get the call's loss afterwards; every
    window equals BAProblem(loss="cauchy") alone, bit for bit; a later stage()
    without the keyword is plain."""
    import torch
    from slam355 import ba

    inp, probs = stage_inputs([outlier_case(6, 150, 4), outlier_case(6, 150, 1)], 6)
    s = torch.cuda.Stream()
    ws = ba.BAWindowSet()
    for kw in (dict(loss="cauchy", f_scale=DELTA), dict()):
        got = ws.stage(*inp, stream=s, **kw)
        code = ba.LOSSES[kw.get("loss", "linear")]
        assert all(p._s.loss == code and p._s.loss_scale == kw.get("f_scale", 1.0) for p in got)
        with torch.cuda.stream(s):
            ba.BABatch(got, stream=s).iterate(4)
        torch.cuda.synchronize()
        for pr, p in zip(probs, got):
            ref = ba.BAProblem(*pr, **kw)
            ref.iterate(4)
            assert ref.state() == p.state()
            for x, y in zip(ref.params(), p.params()):
                assert np.array_equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("loss,scale", [(7, 1.5), (1, 0.0)])
def test_gpu_bad_descriptor_is_refused(loss, scale):
    """A live problem's descriptor with loss = 7, or huber with loss_scale = 0,
    set through the raw struct: the launch returns non-zero with a message
    and nothing is launched (the LM state does not move)."""
    import torch
    from slam355 import _lib, ba

    c0, p0, ci, pi, qs = outlier_case(6, 150, 4)
    prob = ba.BAProblem(c0, p0, ci, pi, qs)
    prob.iterate(1)
    before = prob.t["state"].cpu().numpy().copy()
    bad = _lib.BAProblemStruct()
    ctypes.memmove(ctypes.byref(bad), ctypes.byref(prob._s), ctypes.sizeof(bad))
    bad.loss, bad.loss_scale = loss, scale
    for fn, args in (("slam_ba_iterate", (1, None)), ("slam_ba_iterate_batch", (1, 1, None)),
                     ("slam_ba_build_system", (None,)), ("slam_ba_solve_step", (None,))):
        assert getattr(_lib.lib, fn)(ctypes.byref(bad), *args) != 0
        assert "loss" in _lib.lib.slam_last_error().decode()
    with pytest.raises(_lib.SlamError, match="loss"):
        _lib.call("slam_ba_iterate", ctypes.byref(bad), 1, None)
    torch.cuda.synchronize()
    assert np.array_equal(prob.t["state"].cpu().numpy(), before)
    prob.iterate(1)  # the good descriptor still runs
    assert prob.state()["ITERS"] == 2.0


@pytest.mark.gpu
def test_gpu_bundle_adjustment_loss_keyword():
    """The BundleAdjustment mirror passes loss / f_scale through: the returned
    residuals are raw, and with 10 % wrong matches the inliers end closer to
    their observations under huber than under the plain loss."""
    from slam355 import BundleAdjustment as B

    c0, p0, ci, pi, qs = outlier_case(6, 150, 4)
    clean = make_problem(3, 6, 150, 4)[4]
    inl = np.all(clean == qs, axis=1)
    assert 0.8 < inl.mean() < 0.95
    err = {}
    for loss in (None, "huber"):
        _, rf, x = B.bundle_adjustment(c0, p0, ci, pi, qs, loss=loss, f_scale=DELTA)
        raw = oba.objective(x, 6, 150, ci, pi, qs)
        assert np.allclose(rf, raw, rtol=1e-9, atol=1e-9)
        err[loss] = np.linalg.norm(rf.reshape(-1, 2)[inl], axis=1).mean()
    print(f"mean inlier reprojection error: linear {err[None]:.3f} px, huber {err['huber']:.3f} px")
    assert err["huber"] < err[None]
    _, rf2, x2 = B.bundle_adjustment_with_sparsity(c0, p0, ci, pi, qs, None, loss="huber", f_scale=DELTA)
    assert np.array_equal(x2, x) and np.array_equal(rf2, rf)


# ----------------------------------------------------------------------------- sharded
# pseed of the two sharded shapes: in 1..8, chosen because the Schur reference meets the
# |rho| >= 0.05 precondition in all six huber iterations (checked in the test)
SHARD_PSEED = {(8, 600): 1, (30, 1500): 1}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gpu_worker(rank, world, port, out, C, P, pseed, iters):
    """test_dist._gpu_worker with the outlier case and huber on every rank."""
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "slam-1_amd")]
    import torch
    import torch.distributed as dist
    from slam355.ba import BAProblem, upper_blocks
    from slam355.dist import shard_by_anchor

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    c0, p0, ci, pi, qs = outlier_case(C, P, pseed)
    mine, keep, lpi = shard_by_anchor(len(c0), len(p0), ci, pi, rank, world)
    prob = BAProblem(c0, p0[mine], ci[keep], lpi, qs[keep], lam0=LAM0, block_list=upper_blocks(C, ci, pi),
                     loss="huber", f_scale=DELTA)
    costs = []
    for _ in range(iters):
        prob.step_distributed()
        costs.append(prob.state()["COST_NEW"])
    cams, _ = prob.params()
    if rank == 0:
        np.savez(out, costs=np.array(costs), cams=cams)
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("C,P", [(8, 600), (30, 1500)])
def test_gpu_step_distributed_with_loss_matches_single_rank(tmp_path, C, P):
    """Two landmark shards (gloo, both on device 0), huber on both ranks, 6
    iterations: the all-reduced system and the all-reduced robust trial cost
    follow the single-rank problem (dense system and one-workgroup solve at
    C = 8, packed system and tiled solve at C = 30), at the bars of
    test_dist.test_gpu_step_distributed_matches_single_rank."""
    import torch.multiprocessing as mp
    from slam355.ba import BAProblem

    pseed, iters = SHARD_PSEED[(C, P)], 6
    ref = reference(C, P, pseed, "huber", iters, schur=True)  # asserts the precondition
    c0, p0, ci, pi, qs = ref[0]
    prob = BAProblem(c0, p0, ci, pi, qs, lam0=LAM0, loss="huber", f_scale=DELTA)
    costs = []
    for _ in range(iters):
        prob.iterate(1)
        costs.append(prob.state()["COST_NEW"])
    cams, _ = prob.params()
    assert np.allclose(costs, [r[1] for r in ref[2]], rtol=1e-8)  # and both follow the reference
    out = str(tmp_path / "d.npz")
    del prob
    mp.spawn(_gpu_worker, args=(2, _free_port(), out, C, P, pseed, iters), nprocs=2, join=True)
    d = np.load(out)
    print("single rank", costs, "sharded", d["costs"].tolist())
    assert np.allclose(d["costs"], costs, rtol=1e-8)
    assert np.allclose(d["cams"], cams, rtol=1e-6, atol=1e-9)
