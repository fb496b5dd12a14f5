"""k_lin_mfma's per-point phases on all lanes: a lane per (point, component) for
V and g, a lane per (point, camera slot, half) for the W / Y operand planes
(which are no longer zeroed per chunk: every row below 9m is written, rows from
9m on are zeroed once per workgroup).

Each case is the smallest window at which one of the lane mappings can go
wrong.  Three LM iterations of BAProblem (lin_mode mfma) are compared with the
oracle's Schur LM (oracle.ba.lm_iteration_schur) at the bars of
tests/test_ba.py::test_gpu_lm_iterates_match_oracle: accept flags equal, cost
rel 1e-9, lambda rel 1e-6, parameters rtol 1e-6 / atol 1e-9.  The batched case
is bit-equal to the same windows solved one by one."""
import numpy as np
import pytest

from oracle import ba as oba

ITERS = 3


def _track_problem(seed, C, P, k):
    from slam355.synthetic import ba_problem

    return ba_problem(np.random.default_rng(seed), C, P, k)


def _mixed_tracks(seed=31):
    """One 8-camera window with 20 points seen by camera 0 only (10 of them
    twice: runs of length 2 and nothing else), 6 points with a single
    observation by some other camera, 6 four-view points that one of their
    cameras sees twice (the (c, c) block rows), and 48 plain four-view points."""
    cams, X, ci, pi, qs = _track_problem(seed, 8, 300, 4)
    rng = np.random.default_rng(seed + 1)
    anchor = np.full(300, 99)
    np.minimum.at(anchor, pi, ci)
    only0 = np.nonzero(anchor == 0)[0][:20]
    rest = np.setdiff1d(np.arange(300), np.nonzero(anchor == 0)[0])[:60]
    keep = np.isin(pi, rest) | (np.isin(pi, only0) & (ci == 0))
    for p in rest[:6]:
        keep[np.nonzero(pi == p)[0][1:]] = False
    ci, pi, qs = ci[keep], pi[keep], qs[keep]
    dup = np.concatenate([np.nonzero(np.isin(pi, only0[:10]))[0],
                          [np.nonzero(pi == p)[0][0] for p in rest[6:12]]]).astype(np.int64)
    ci, pi = np.append(ci, ci[dup]), np.append(pi, pi[dup])
    qs = np.vstack([qs, qs[dup] + rng.normal(0, 0.5, (len(dup), 2))])
    sel = np.concatenate([only0, rest])
    remap = np.full(300, -1)
    remap[sel] = np.arange(len(sel))
    return cams, X[sel], ci, remap[pi], qs


def _case(name):
    """(problem, start, BAProblem keywords, lam0)"""
    from slam355 import ba
    from slam355.synthetic import perturb

    kw, lam0, start = {}, 1e-4, (1e-3, 1e-2, 0.05)
    if name == "full_chunk":  # 7 cameras x 16 points, all see all: 112 obs, m = 7, only row 63 unwritten
        prob = _track_problem(41, 7, 16, 7)
        kw = dict(chunks_per_wg=1)
    elif name in ("six_views", "held", "rejected"):  # m = 6 and 7 supergroups, rows 54..63 unwritten
        prob = _track_problem(12, 10, 40, 6)
        if name == "held":
            kw = dict(fixed=ba.FIXED_INTRINSICS)
        if name == "rejected":
            # three times the usual start noise: the oracle turns the third step
            # down (rho = -0.12).  Chosen on the CPU among starts at which the
            # oracle's two formulations (lm_iteration, lm_iteration_schur)
            # agree to 1e-10 in the trial cost -- at lambda0 <= 1e-6 they
            # differ by 2e-9 themselves, more than the bar.
            start = (3e-3, 3e-2, 0.15)
    elif name == "mixed":
        prob = _mixed_tracks()
        kw = dict(chunks_per_wg=1)
    elif name == "npts_varies":  # chunks of 16, 16, 5 points in one workgroup
        prob = _track_problem(21, 7, 37, 4)
        kw = dict(chunks_per_wg=3)
    else:
        raise KeyError(name)
    seed = 14 if name == "rejected" else 7
    c0, p0 = perturb(np.random.default_rng(seed), prob[0], prob[1], *start)
    return prob, (c0, p0), kw, lam0


def _check_plan(name, prob, plan):
    ci, pi = prob[2], prob[3]
    m = plan["sg_meta"].reshape(-1, 24)[:, 3]
    npts = np.diff(plan["grp_ptr"])
    if name == "full_chunk":
        assert len(ci) == 112 and list(npts) == [16] and list(m) == [7]
    elif name == "mixed":
        assert 1 in m and m.max() > 1                       # a one-camera supergroup, and others
        assert (np.bincount(pi) == 1).sum() >= 6            # single observations
        o = np.lexsort((ci, pi))
        run2 = (ci[o][1:] == ci[o][:-1]) & (pi[o][1:] == pi[o][:-1])
        assert run2.sum() == 16                             # a camera sees a point twice
    elif name == "npts_varies":
        assert list(npts) == [16, 16, 5] and plan["n_sgrps"] == 1
    else:
        assert {6, 7} <= set(m.tolist())


_ORACLE = {}  # case -> per-iteration oracle records, computed once


def _oracle(name, monkeypatch):
    if name in _ORACLE:
        return _ORACLE[name]
    from slam355 import ba

    (cams, pts, ci, pi, qs), (c0, p0), kw, lam0 = _case(name)
    if "fixed" in kw:  # the oracle with the held columns of Jc zeroed (as tests/test_ba_fixed.py)
        words = ba.fixed_mask(len(cams), kw["fixed"])
        held = ((np.asarray(words)[:, None] >> np.arange(9, dtype=np.uint32)) & 1).astype(bool)
        orig = oba.residual_and_jacobian

        def masked(cams_, pts_, cam_idx, pt_idx, qs_):
            r, J = orig(cams_, pts_, cam_idx, pt_idx, qs_)
            J = J.copy()
            h = held[np.asarray(cam_idx)]
            J[:, :, :9][np.broadcast_to(h[:, None, :], J[:, :, :9].shape)] = 0.0
            return r, J

        monkeypatch.setattr(oba, "residual_and_jacobian", masked)
    st = oba.LMState(lam0)
    oc, op = c0.copy(), p0.copy()
    pairs = oba._obs_pairs(ci, pi)
    recs = []
    for _ in range(ITERS):
        oc, op, info = oba.lm_iteration_schur(oc, op, ci, pi, qs, st, pairs)
        assert abs(info["rho"]) >= 0.05, (name, info)  # the decision is not a matter of rounding
        recs.append((bool(info["accepted"]), info["cost_new"], st.lam, oc.copy(), op.copy()))
    _ORACLE[name] = recs
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["full_chunk", "six_views", "mixed", "npts_varies", "held", "rejected"])
def test_gpu_lane_mappings_match_oracle(name, monkeypatch):
    from slam355 import ba

    prob, (c0, p0), kw, lam0 = _case(name)
    recs = _oracle(name, monkeypatch)
    if name == "rejected":  # the oracle turns at least one of the steps down
        assert not all(r[0] for r in recs) and any(r[0] for r in recs)
    g = ba.BAProblem(c0, p0, *prob[2:], lin_mode="mfma", lam0=lam0, **kw)
    assert g.lin_mode == "mfma"
    _check_plan(name, prob, g.plan)
    for it, (acc, cost_new, lam, oc, op) in enumerate(recs):
        g.iterate(1)
        s = g.state()
        gc, gp = g.params()
        print(f"{name} it {it}: accepted {s['ACCEPTED']:.0f}/{acc} cost rel "
              f"{abs(s['COST_NEW'] - cost_new) / cost_new:.2e} lambda rel {abs(s['LAMBDA'] - lam) / lam:.2e} "
              f"cams {np.abs(gc - oc).max():.2e} pts {np.abs(gp - op).max():.2e}")
        assert bool(s["ACCEPTED"]) == acc, it
        assert abs(s["COST_NEW"] - cost_new) <= 1e-9 * cost_new + 1e-12, it
        assert abs(s["LAMBDA"] - lam) <= 1e-6 * lam, it
        assert np.allclose(gc, oc, rtol=1e-6, atol=1e-9), it
        assert np.allclose(gp, op, rtol=1e-6, atol=1e-9), it


@pytest.mark.gpu
def test_gpu_batch_of_unequal_windows_equals_single_windows():
    """Three windows of 1, 5 and 3 supergroups in one BABatch (grid.x covers the
    largest; the others' surplus workgroups return at once): bit-equal to the
    windows solved one by one."""
    from slam355 import ba

    names = ["full_chunk", "mixed", "six_views"]
    cases = [_case(n) for n in names]
    mk = lambda: [ba.BAProblem(c0, p0, *prob[2:], lin_mode="mfma", lam0=lam0, **kw)  # noqa: E731
                  for prob, (c0, p0), kw, lam0 in cases]
    single, batched = mk(), mk()
    assert len({p.plan["n_sgrps"] for p in single}) == len(single)  # all sizes differ
    batch = ba.BABatch(batched)
    batch.iterate(ITERS)
    for a, b in zip(single, batched):
        a.iterate(ITERS)
        assert a.state() == b.state()
        for x, y in zip(a.params(), b.params()):
            assert np.array_equal(x, y)
