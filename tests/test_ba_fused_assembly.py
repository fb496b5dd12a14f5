"""k_solve_blk<true>: the one-workgroup camera solve sums the lineariser's
partial rows itself (csrc/ba_solve.hip, asm_prologue), so slam_ba_iterate /
slam_ba_iterate_batch launch no k_assemble.  The prologue walks k_assemble's
1024-lane summation order on the solve's 256 lanes, so nothing may differ by a
bit -- not even the sign of a zero.

The reference of every case is the step-wise API on a twin problem
(build_system(), solve_step(), decide()), which keeps the k_assemble launch.
After each of 3 LM iterations the bytes of sys, of the LM state and of the
parameters are compared; iterate() with the switch off must give them too.
Each case asserts from its plan that it has the shape it is meant to have:

  deep        2 cameras x 1600 points x 2 views, one chunk per workgroup: 100
              partial rows per camera and per block, so both row widths run
              the 8-deep trip and the remainder (109 wide: 9 parts, 81 wide:
              12 parts)
  empty       6 cameras, points seen by neighbouring cameras only: off-diagonal
              blocks without rows (-0.0 in S, both mirrored entries)
  twice       points observed twice by one camera, lin_mode="slot" (the plan
              that gives them block rows of (c, c)): B + B^T on the diagonal
  largest     13 cameras (9C = 117): 91 blocks, the staging at its largest,
              rows >= 64 of the back substitution
  sg_edge     8 cameras x 400 points x 6 views: several supergroups that share
              cameras
  robust      sg_edge with loss="huber" (the cost entry e = 108)
  slot        empty with lin_mode="slot" (k_linearize's partial rows)
  failed      empty with lambda = -1e6: the factor fails, a zero step
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ITERS = 3
CASES = ["deep", "empty", "twice", "largest", "sg_edge", "robust", "slot", "failed"]


def _tracks_window(seed, C, tracks):
    """Cameras and points of synthetic.ba_problem observed as `tracks` says (one
    camera list per point; a camera listed twice sees the point twice)."""
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
    """(cams0, pts0, cam_idx, pt_idx, qs, BAProblem keywords, lambda0)"""
    from slam355.synthetic import ba_problem, perturb

    kw, lam0 = dict(lin_mode="mfma"), 1e-4
    if name == "deep":
        cams, pts, ci, pi, qs = ba_problem(np.random.default_rng(11), 2, 1600, 2)
        kw["chunks_per_wg"] = 1
    elif name in ("empty", "slot", "failed"):
        cams, pts, ci, pi, qs = ba_problem(np.random.default_rng(12), 6, 300, 2)
        if name == "slot":
            kw["lin_mode"] = "slot"
        if name == "failed":
            lam0 = -1e6
    elif name == "twice":
        tr = [[a, a, a + 1, a + 2] for a in (0, 1, 2)] + [[a, a + 1, a + 2] for a in (0, 1, 2)]
        cams, pts, ci, pi, qs = _tracks_window(13, 5, [t for t in tr for _ in range(40)])
        kw["lin_mode"] = "slot"  # k_lin_mfma takes T_aa into the camera row: only the slot plan has (c, c) rows
    elif name == "largest":
        cams, pts, ci, pi, qs = ba_problem(np.random.default_rng(14), 13, 300, 4)
    elif name in ("sg_edge", "robust"):
        cams, pts, ci, pi, qs = ba_problem(np.random.default_rng(15), 8, 400, 6)
        if name == "robust":
            kw.update(loss="huber", f_scale=1.0)
    else:
        raise KeyError(name)
    c0, p0 = perturb(np.random.default_rng(7), cams, pts)
    return c0, p0, ci, pi, qs, kw, lam0


def _check_plan(name, prob):
    pl = prob.plan
    blocks = np.asarray(pl["blocks"]).reshape(-1, 2)
    crows = np.diff(pl["cam_cslot_ptr"])
    brows = np.diff(pl["blk_bslot_ptr"])
    diag = blocks[:, 0] == blocks[:, 1]
    C = prob.C
    assert len(blocks) == C * (C + 1) // 2  # dense: every upper block listed
    assert prob.lin_mode == ("slot" if name in ("slot", "twice") else "mfma")
    if name == "deep":
        assert crows.max() > 72 and brows.max() > 96
        # neither a multiple of the 8-deep trip: 9 * 8 = 72 and 12 * 8 = 96 rows
        assert crows.max() % 72 and brows.max() % 96
    elif name in ("empty", "slot", "failed"):
        assert C == 6 and (brows[~diag] == 0).any() and (brows[~diag] > 0).any()
    elif name == "twice":
        assert (brows[diag] > 0).any()
    elif name == "largest":
        assert C == 13 and len(blocks) == 91
    else:
        assert C == 8
        meta = np.asarray(pl["sg_meta"]).reshape(-1, 24)
        assert len(meta) > 1
        sets = [set(r[10:10 + r[3]].tolist()) for r in meta]
        assert any(sets[i] & sets[j] for i in range(len(sets)) for j in range(i))


def _snap(prob):
    """bytes of sys, LM state and live parameters (state() raises on a solve fault)"""
    import torch

    torch.cuda.synchronize()
    st = prob.state()
    c, p = prob.params()
    return (prob.t["sys"].cpu().numpy().tobytes(), prob.t["state"].cpu().numpy().tobytes(),
            c.tobytes(), p.tobytes()), st


FORCED = 2  # fused whatever the window's row count (1, the default, fuses up to 1024 partial rows)


def _fused(on):
    from slam355 import _lib

    _lib.call("slam_ba_set_fused_assembly", int(on))


def _make(name):
    from slam355 import ba

    c0, p0, ci, pi, qs, kw, lam0 = _case(name)
    prob = ba.BAProblem(c0, p0, ci, pi, qs, **kw)
    if lam0 != 1e-4:
        prob.reset(lam0)
    return prob


_REF = {}  # case -> per-iteration (bytes, state) of the step-wise run, computed once


def _reference(name):
    if name not in _REF:
        prob = _make(name)
        _check_plan(name, prob)
        rows = []
        for _ in range(ITERS):
            prob.build_system()
            prob.solve_step()
            prob.decide()
            rows.append(_snap(prob))
        _REF[name] = rows
    return _REF[name]


def _iterate_rows(name, on):
    _fused(on)
    try:
        prob = _make(name)
        rows = []
        for _ in range(ITERS):
            prob.iterate(1)
            rows.append(_snap(prob))
    finally:
        _fused(1)
    return rows


WHAT = ("sys", "state", "cams", "pts")


def _assert_rows(got, ref, tag):
    for it, ((gb, _), (rb, _)) in enumerate(zip(got, ref)):
        for w, g, r in zip(WHAT, gb, rb):
            if g != r:
                ga, ra = np.frombuffer(g, np.uint64), np.frombuffer(r, np.uint64)
                bad = np.flatnonzero(ga != ra)
                raise AssertionError(f"{tag}: {w} differs at iteration {it}: {len(bad)} of {len(ga)} "
                                     f"words, first at {bad[:8].tolist()}")


@pytest.mark.parametrize("name", CASES)
def test_gpu_fused_assembly_equals_stepwise(name):
    """iterate() with the fused solve gives the bytes of build_system() +
    solve_step() + decide() after every iteration; so does iterate() with the
    switch off."""
    ref = _reference(name)
    if name == "failed":
        assert all(st["CHOL_FAIL"] == 1.0 and st["ACCEPTED"] == 0.0 for _, st in ref)
    else:
        assert any(st["ACCEPTED"] == 1.0 for _, st in ref), "the reference accepted no step: pick another seed"
        assert all(st["CHOL_FAIL"] == 0.0 for _, st in ref)
    on = _iterate_rows(name, FORCED)
    _assert_rows(on, ref, "fused on vs step-wise")
    _assert_rows(_iterate_rows(name, 1), ref, "fused by default vs step-wise")
    off = _iterate_rows(name, 0)
    _assert_rows(off, ref, "fused off vs step-wise")
    if name in ("empty", "slot"):  # the signed zeros are there to be compared
        S = np.frombuffer(ref[0][0][0], np.float64)
        assert (np.signbit(S) & (S == 0.0)).any()
    if name == "failed":
        prob = _make(name)
        c_before, p_before = prob.params()
        prob.iterate(1)
        c, p = prob.params()
        assert np.array_equal(c, c_before) and np.array_equal(p, p_before)
        assert not prob.t["delta_c"].cpu().numpy().any()


def test_gpu_fused_assembly_batch():
    """BABatch of the 13-, 2- and 8-camera windows (different n, 63 KB / 4 KB /
    27 KB of LDS layout in one launch): fused equals the step-wise twins, the
    unfused batch and the windows iterated one by one."""
    from slam355 import ba

    names = ["largest", "deep", "sg_edge"]
    refs = [_reference(n) for n in names]
    for on in (FORCED, 0):
        _fused(on)
        try:
            probs = [_make(n) for n in names]
            batch = ba.BABatch(probs)
            for it in range(ITERS):
                batch.iterate(1)
                for n, p, ref in zip(names, probs, refs):
                    _assert_rows([_snap(p)], [ref[it]], f"batch ({'on' if on else 'off'}) {n} iteration {it}")
        finally:
            _fused(1)
    for n, ref in zip(names, refs):
        _assert_rows(_iterate_rows(n, FORCED), ref, f"solo {n}")


def test_gpu_fused_assembly_switch_between_iterations():
    """The switch is read when launches are issued: off, then on, then forced
    between the iterate() calls of one problem gives the bytes of an
    uninterrupted run."""
    ref = _reference("sg_edge")
    prob = _make("sg_edge")
    rows = []
    try:
        for on in (0, 1, FORCED)[:ITERS]:
            _fused(on)
            prob.iterate(1)
            rows.append(_snap(prob))
    finally:
        _fused(1)
    _assert_rows(rows, ref, "switched")
    from slam355 import _lib

    with pytest.raises(_lib.SlamError):
        _lib.call("slam_ba_set_fused_assembly", 3)
