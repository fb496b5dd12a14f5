"""k_lin_mfma's (D) phase with the accumulation units dealt by a fixed table:
the 10 upper tiles of T and the <= 7 camera tiles go to the four waves so that
the waves take equal time (csrc/ba.hip, the deal above linm_schur), a wave's
tiles share a tile row or column, and no wave feeds an accumulator it does not
own.

Each window is the smallest at which the deal or a lane mapping can go wrong:

  m_sweep     supergroups of m = 1, 2, 3, 4, 6, 7, 7 cameras (tile rows nt = 1,
              2, 2, 3, 4, 4, 4), 16 points each: waves with 0 to 5 units,
              every variant of the tile and camera loops, cameras past m
  held        the same window with fixed=FIXED_INTRINSICS (the `held` path)
  one_point   1 point seen by 7 cameras: 3 of the 16 K-steps of one MFMA group
  five_points 5 points seen by 7 cameras: 15 of 16 K-steps
              (windows this small leave free cameras undetermined and the cost
              goes to zero, where the oracle's own two formulations differ by
              more than the bars; so one_point holds its cameras whole and
              five_points their intrinsics, which makes them determined)
  k_tail      16 + 16 + 3 points in one workgroup (3 npts = 9 in the last
              chunk), camera 0 without observations in chunks 2 and 3, every
              camera of chunk 3 with an odd count (the Z pair tail)
  full_obs    chunks of exactly kMObs = 120 observations (15 points x 8, camera
              0 sees every point twice: runs of length 2), two supergroups

Three LM iterations of BAProblem (lin_mode mfma), so accepted steps re-enter
the kernel, against
  * the oracle's Schur LM at the bars of tests/test_ba_lanes.py: accept flags
    equal, cost rel 1e-9, lambda rel 1e-6, parameters rtol 1e-6 / atol 1e-9;
  * lin_mode "slot" on the same window at the same bars: the slot kernel is the
    same LM with the sums taken in another order, which is what those bars
    were set for.
The folded assembly, the batch and the repeated run are compared bit for bit."""
import numpy as np
import pytest

from oracle import ba as oba

ITERS = 3
NAMES = ["m_sweep", "held", "one_point", "five_points", "k_tail", "full_obs"]


def _window(seed, C, tracks):
    """Cameras and points of synthetic.ba_problem, observed as `tracks` says
    (one camera list per point; a camera listed twice sees the point twice)."""
    from slam355.synthetic import ba_problem, bal_project

    rng = np.random.default_rng(seed)
    cams, X, _, _, _ = ba_problem(rng, C, len(tracks), 1)
    ci = np.concatenate([np.asarray(t, np.int64) for t in tracks])
    pi = np.repeat(np.arange(len(tracks)), [len(t) for t in tracks])
    o = rng.permutation(len(ci))
    ci, pi = ci[o], pi[o]
    qs = bal_project(X[pi], cams[ci]) + rng.normal(0, 0.5, (len(ci), 2))
    return cams, X, ci, pi, qs


def _case(name):
    """(problem, start, BAProblem keywords)"""
    from slam355 import ba
    from slam355.synthetic import perturb

    kw = dict(chunks_per_wg=1)
    if name in ("m_sweep", "held"):
        sets = [[0], [0, 1], [0, 1, 2], [0, 1, 2, 3], list(range(6)), list(range(7)), list(range(1, 8))]
        prob = _window(51, 8, [s for s in sets for _ in range(16)])
        if name == "held":
            kw["fixed"] = ba.FIXED_INTRINSICS
    elif name == "one_point":  # every camera held whole: 14 residuals for the point's 3 unknowns
        prob = _window(52, 7, [list(range(7))])
        kw["fixed"] = ba.FIXED_CAMERA
    elif name == "five_points":  # intrinsics held: 70 residuals for 57 unknowns
        prob = _window(53, 7, [list(range(7))] * 5)
        kw["fixed"] = ba.FIXED_INTRINSICS
    elif name == "k_tail":
        prob = _window(54, 6, [list(range(a, a + 4)) for a in [0] * 16 + [1] * 16 + [2] * 3])
        kw = dict(chunks_per_wg=3)
    elif name == "full_obs":
        prob = _window(55, 7, [[0] + list(range(7))] * 30)
    else:
        raise KeyError(name)
    c0, p0 = perturb(np.random.default_rng(7), prob[0], prob[1])
    return prob, (c0, p0), kw


def _check_plan(name, plan):
    meta = plan["sg_meta"].reshape(-1, 24)
    m = meta[:, 3].tolist()
    npts = np.diff(plan["grp_ptr"]).tolist()
    nobs = np.diff(plan["chk_optr"]).tolist()
    runs = np.diff(plan["chk_cptr"].reshape(-1, 8), axis=1)  # [chunk][camera slot]
    if name in ("m_sweep", "held"):
        assert m == [1, 2, 3, 4, 6, 7, 7] and npts == [16] * 7
    elif name == "one_point":
        assert m == [7] and npts == [1]
    elif name == "five_points":
        assert m == [7] and npts == [5]
    elif name == "k_tail":
        assert m == [6] and npts == [16, 16, 3]
        assert runs[1, 0] == 0 and runs[2, 0] == 0      # camera 0 is absent from chunks 2 and 3
        assert (runs[2, 2:6] == 3).all()                # odd counts
    else:
        assert m == [7, 7] and npts == [15, 15] and nobs == [120, 120]
        assert (runs[:, 0] == 30).all() and (runs[:, 1:7] == 15).all()


_ORACLE = {}  # case -> per-iteration oracle records, computed once


def _oracle(name, monkeypatch):
    if name in _ORACLE:
        return _ORACLE[name]
    from slam355 import ba

    (cams, pts, ci, pi, qs), (c0, p0), kw = _case(name)
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
    st = oba.LMState(1e-4)
    oc, op = c0.copy(), p0.copy()
    pairs = oba._obs_pairs(ci, pi)
    recs = []
    for _ in range(ITERS):
        oc, op, info = oba.lm_iteration_schur(oc, op, ci, pi, qs, st, pairs)
        assert abs(info["rho"]) >= 0.05, (name, info)  # the decision is not a matter of rounding
        recs.append((bool(info["accepted"]), info["cost_new"], st.lam, oc.copy(), op.copy()))
    _ORACLE[name] = recs
    return recs


def _gpu(name, **over):
    from slam355 import ba

    prob, (c0, p0), kw = _case(name)
    return ba.BAProblem(c0, p0, *prob[2:], **{"lin_mode": "mfma", "lam0": 1e-4, **kw, **over})


def _records(g):
    recs = []
    for _ in range(ITERS):
        g.iterate(1)
        s = g.state()
        gc, gp = g.params()
        recs.append((bool(s["ACCEPTED"]), s["COST_NEW"], s["LAMBDA"], gc, gp))
    return recs


_MFMA = {}  # case -> per-iteration records of the mfma run, computed once


def _mfma(name):
    if name not in _MFMA:
        g = _gpu(name)
        assert g.lin_mode == "mfma"
        _check_plan(name, g.plan)
        _MFMA[name] = _records(g)
    return _MFMA[name]


def _assert_close(name, what, got, want):
    for it, ((ga, gcost, glam, gc, gp), (acc, cost_new, lam, oc, op)) in enumerate(zip(got, want)):
        print(f"{name} vs {what} it {it}: accepted {ga}/{acc} cost rel {abs(gcost - cost_new) / cost_new:.2e} "
              f"lambda rel {abs(glam - lam) / lam:.2e} cams {np.abs(gc - oc).max():.2e} "
              f"pts {np.abs(gp - op).max():.2e}")
        assert ga == acc, it
        assert abs(gcost - cost_new) <= 1e-9 * cost_new + 1e-12, it
        assert abs(glam - lam) <= 1e-6 * lam, it
        assert np.allclose(gc, oc, rtol=1e-6, atol=1e-9), it
        assert np.allclose(gp, op, rtol=1e-6, atol=1e-9), it


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_wave_deal_matches_oracle(name, monkeypatch):
    _assert_close(name, "oracle", _mfma(name), _oracle(name, monkeypatch))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_wave_deal_matches_slot_kernel(name):
    g = _gpu(name, lin_mode="slot")
    assert g.lin_mode == "slot"
    _assert_close(name, "slot", _mfma(name), _records(g))


@pytest.mark.gpu
def test_gpu_folded_assembly_equals_separate_launch():
    """full_obs: two supergroups, so every camera block has two partial rows and
    every pair block two.  With at most two rows per block the folded sum
    (rows dealt over kFoldWG / n parts, parts added in order) and k_assemble's
    (its own part count) add the same two numbers in the same order, so the two
    launches must agree bit for bit -- the reduced system after one build, and
    every state and parameter of three iterations.  (More rows per block: equal
    to rounding only, tests/test_ba.py.)"""
    a, b = _gpu("full_obs", fold_assembly=True), _gpu("full_obs")
    assert "asm_tab" in a.t and "asm_tab" not in b.t and a.plan["n_sgrps"] == 2
    assert np.diff(a.plan["cam_cslot_ptr"]).max() == 2 and np.diff(a.plan["blk_bslot_ptr"]).max() == 2
    a.build_system()
    b.build_system()
    assert np.array_equal(a.t["sys"].cpu().numpy(), b.t["sys"].cpu().numpy())
    for (fa, fcost, flam, fc, fp), (ua, ucost, ulam, uc, up) in zip(_records(a), _records(b)):
        assert (fa, fcost, flam) == (ua, ucost, ulam)
        assert np.array_equal(fc, uc) and np.array_equal(fp, up)


@pytest.mark.gpu
def test_gpu_batch_equals_single_windows_and_repeats():
    """Three windows of 7, 1 and 2 supergroups in one BABatch: bit-equal to the
    windows solved one by one; and a second run of the same windows repeats the
    first bit for bit (the deal is fixed: no order dependence)."""
    from slam355 import ba

    names = ["m_sweep", "k_tail", "full_obs"]
    single, batched, again = ([_gpu(n) for n in names] for _ in range(3))
    assert [p.plan["n_sgrps"] for p in single] == [7, 1, 2]
    ba.BABatch(batched).iterate(ITERS)
    for n, a, b, c in zip(names, single, batched, again):
        a.iterate(ITERS)
        c.iterate(ITERS)
        assert a.state() == b.state() == c.state(), n
        for x, y, z in zip(a.params(), b.params(), c.params()):
            assert np.array_equal(x, y) and np.array_equal(x, z), n
