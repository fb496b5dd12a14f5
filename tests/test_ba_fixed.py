"""Bundle adjustment with held camera parameters (slam_ba_problem.cam_fixed,
slam355.ba.fixed_mask / BAProblem(fixed=...)).

Semantics: a held parameter's column is removed from the Jacobian; nothing
else about the LM iteration changes.  Reference: the oracle's own LM
(oracle.ba.lm_iteration / lm_iteration_schur) with
oracle.ba.residual_and_jacobian replaced (monkeypatch) by a wrapper that zeroes
the held camera columns of every observation.  That reference leaves held
parameters bit-equal to the input.

Bars (float64), those of tests/test_ba.py's oracle tests: accept flag equal,
COST_NEW 1e-9 relative (tiled solve: 1e-8), lambda 1e-6 relative, cameras and
points rtol 1e-6 / atol 1e-9, held entries np.array_equal to the input.
Precondition (a condition on the reference, not a tolerance): in every
compared iteration the oracle's |rho| >= 0.05, and an accepted step has
rho <= 1.5, so no accept flag is decided by rounding.
"""
import ctypes

import numpy as np
import pytest

from oracle import ba as oba
from stage_ref import stage_inputs, synthetic_windows


def make_problem(seed, C, P, obs_per_pt):
    from slam355.synthetic import ba_problem

    return ba_problem(np.random.default_rng(seed), C, P, obs_per_pt, f=716.8, noise=0.5)


def _perturb(rng, cams, pts):
    """The perturbation of test_gpu_lm_iterates_match_oracle."""
    C = len(cams)
    cams0 = cams.copy()
    cams0[:, :3] += rng.normal(0, 1e-3, (C, 3))
    cams0[:, 3:6] += rng.normal(0, 1e-2, (C, 3))
    return cams0, pts + rng.normal(0, 0.05, pts.shape)


def _held(words):
    """[C, 9] bool from the mask words."""
    return ((np.asarray(words)[:, None] >> np.arange(9, dtype=np.uint32)) & 1).astype(bool)


_ORACLE = {}  # case name -> (problem, start, mask words, per-iteration oracle records)


def _oracle_case(monkeypatch, name, build, iters, schur):
    """The masked oracle LM of one case, computed once per session and shared
    (read-only) by the parametrised tests that compare against it."""
    if name in _ORACLE:
        return _ORACLE[name]
    from slam355 import ba

    prob, (c0, p0), fixed = build()
    cams, pts, ci, pi, qs = prob
    words = ba.fixed_mask(len(cams), fixed)
    orig = oba.residual_and_jacobian

    def masked(cams_, pts_, cam_idx, pt_idx, qs_):
        r, J = orig(cams_, pts_, cam_idx, pt_idx, qs_)
        J = J.copy()
        held = _held(words)[np.asarray(cam_idx)]
        J[:, :, :9][np.broadcast_to(held[:, None, :], J[:, :, :9].shape)] = 0.0
        return r, J

    monkeypatch.setattr(oba, "residual_and_jacobian", masked)
    st = oba.LMState(1e-4)
    oc, op = c0.copy(), p0.copy()
    pairs = oba._obs_pairs(ci, pi) if schur else None
    recs = []
    for _ in range(iters):
        if schur:
            oc, op, info = oba.lm_iteration_schur(oc, op, ci, pi, qs, st, pairs)
        else:
            oc, op, info = oba.lm_iteration(oc, op, ci, pi, qs, st)
        # precondition: the accept decision is not a matter of rounding
        assert abs(info["rho"]) >= 0.05, (name, info)
        assert not info["accepted"] or info["rho"] <= 1.5, (name, info)
        recs.append((bool(info["accepted"]), info["cost_new"], st.lam, oc.copy(), op.copy()))
    h = _held(words)
    assert np.array_equal(oc[h], c0[h])  # the reference itself never moves a held entry
    for a in (c0, p0, words) + tuple(x for r in recs for x in r[3:]):
        a.setflags(write=False)
    _ORACLE[name] = (prob, (c0, p0), words, recs)
    return _ORACLE[name]


def _compare(prob_gpu, case, cost_rtol):
    _, (c0, _), words, recs = case
    h = _held(words)
    assert np.array_equal(prob_gpu.fixed, words)
    for it, (acc, cost_new, lam, oc, op) in enumerate(recs):
        prob_gpu.iterate(1)
        s = prob_gpu.state()
        gc, gp = prob_gpu.params()
        print(f"it {it}: accepted {s['ACCEPTED']:.0f}/{acc} cost_new rel "
              f"{abs(s['COST_NEW'] - cost_new) / cost_new:.2e} lambda rel {abs(s['LAMBDA'] - lam) / lam:.2e} "
              f"cams {np.abs(gc - oc).max():.2e} (rel {np.abs((gc - oc) / np.where(oc == 0, 1, oc)).max():.2e}) "
              f"pts {np.abs(gp - op).max():.2e}")
        assert s["CHOL_FAIL"] == 0.0, it
        assert bool(s["ACCEPTED"]) == acc, it
        assert abs(s["COST_NEW"] - cost_new) <= cost_rtol * cost_new + 1e-12, it
        assert abs(s["LAMBDA"] - lam) <= 1e-6 * lam, it
        assert np.allclose(gc, oc, rtol=1e-6, atol=1e-9), it
        assert np.allclose(gp, op, rtol=1e-6, atol=1e-9), it
        # held entries: bit-identical to the input, in both parameter buffers
        for k in ("cams0", "cams1"):
            assert np.array_equal(prob_gpu.t[k].cpu().numpy()[h], c0[h]), (it, k)


# ----------------------------------------------------------------------------- host
def test_fixed_mask_words():
    from slam355 import ba

    assert ba.fixed_mask(3, ba.FIXED_INTRINSICS).tolist() == [0x1C0] * 3
    assert ba.fixed_mask(3, ba.FIXED_INTRINSICS).dtype == np.uint32
    assert ba.fixed_mask(4, None).tolist() == [0, 0, 0, 0]
    m = np.random.default_rng(0).integers(0, 2, (7, 9))
    for arr in (m, m.astype(bool), m.astype(np.float64)):
        w = ba.fixed_mask(7, arr)
        assert w.shape == (7,) and w.dtype == np.uint32
        assert np.array_equal(_held(w), m.astype(bool))  # round trip, bit by bit
        assert np.all(w < 512)
    assert ba.fixed_mask(2, np.ones(9, bool)).tolist() == [0x1FF, 0x1FF]


@pytest.mark.parametrize("bad", [np.zeros((4, 9)), np.zeros(8), np.zeros((5, 9, 1)), np.zeros((9, 5)),
                                 np.full(9, 2), np.full((5, 9), -1), np.full(9, 0.5), 1])
def test_fixed_mask_rejects_bad_input(bad):
    from slam355 import ba

    with pytest.raises(ValueError):
        ba.fixed_mask(5, bad)


def test_problem_struct_size_matches_library():
    from slam355 import _lib

    assert _lib.lib.slam_ba_problem_size() == ctypes.sizeof(_lib.BAProblemStruct)
    assert _lib.BAProblemStruct._fields_[-1][0] == "cam_fixed"
    assert _lib.BAProblemStruct.cam_fixed.offset == ctypes.sizeof(_lib.BAProblemStruct) - 8


# ----------------------------------------------------------------------------- GPU
def _case_small():
    from slam355 import ba

    cams, pts, ci, pi, qs = make_problem(3, 6, 150, 4)
    fixed = np.tile(ba.FIXED_INTRINSICS, (6, 1))
    fixed[0] = 1     # camera 0 wholly held (gauge)
    fixed[1, 5] = 1  # one more translation component
    return (cams, pts, ci, pi, qs), _perturb(np.random.default_rng(4), cams, pts), fixed


@pytest.mark.gpu
@pytest.mark.parametrize("lin_mode", ["auto", "slot"])
def test_gpu_fixed_small_matches_masked_oracle(monkeypatch, lin_mode):
    """One-workgroup solve, both linearisations (k_lin_mfma under "auto",
    k_linearize under "slot"): 6 LM iterates equal the dense masked oracle."""
    from slam355 import ba

    case = _oracle_case(monkeypatch, "small", _case_small, 6, schur=False)
    (_, _, ci, pi, qs), (c0, p0), words, _ = case
    prob = ba.BAProblem(c0, p0, ci, pi, qs, lin_mode=lin_mode, fixed=_held(words))
    assert prob.lin_mode == ("slot" if lin_mode == "slot" else "mfma")
    _compare(prob, case, 1e-9)


def _case_tiled():
    from slam355 import ba

    cams, pts, ci, pi, qs = make_problem(3, 14, 400, 4)
    fixed = np.tile(ba.FIXED_INTRINSICS, (14, 1))
    fixed[0] = fixed[13] = 1
    return (cams, pts, ci, pi, qs), _perturb(np.random.default_rng(4), cams, pts), fixed


@pytest.mark.gpu
@pytest.mark.parametrize("tl_mode", ["flow", "levels"])
def test_gpu_fixed_tiled_solve_matches_masked_oracle(monkeypatch, tl_mode):
    """9C = 126 > 120: the tiled camera solve (dataflow and level-scheduled),
    intrinsics held and cameras 0 and 13 held whole; 8 LM iterates equal the
    masked oracle's Schur LM, accept flag by accept flag (the oracle accepts
    all 8 from this start; rejected steps are compared in the deep-loop test)."""
    from slam355 import ba

    case = _oracle_case(monkeypatch, "tiled", _case_tiled, 8, schur=True)
    (_, _, ci, pi, qs), (c0, p0), words, _ = case
    prob = ba.BAProblem(c0, p0, ci, pi, qs, tl_mode=tl_mode, fixed=_held(words))
    assert prob.tl_levels
    _compare(prob, case, 1e-9)


def _case_loop(C, P, k):
    def build():
        from slam355 import ba
        from slam355.synthetic import ba_problem_loop

        rng = np.random.default_rng(5)
        cams, pts, ci, pi, qs = ba_problem_loop(rng, C, P, k)
        return (cams, pts, ci, pi, qs), _perturb(rng, cams, pts), ba.FIXED_INTRINSICS
    return build


@pytest.mark.gpu
@pytest.mark.parametrize("C,P,k,tiles,lin", [(60, 3000, 8, "rows64", "slot"), (40, 2000, 7, "cams:3", "mfma")])
def test_gpu_fixed_deep_loops_flow_solve_matches_masked_oracle(monkeypatch, C, P, k, tiles, lin):
    """The closed loops of test_gpu_flow_product_tasks_of_deeper_rows_equal_level_solve
    (7-8 views per point: the dataflow solve's reload product tasks run), with
    the intrinsics held: the reduced system's condition number drops from
    1e23-1e29 to ~1e7, so the dataflow camera solve is compared with the
    oracle's Schur LM itself, at the bars of
    test_gpu_tiled_solver_iterates_match_oracle, over 4 iterations (accepted
    and rejected steps both occur)."""
    from slam355 import ba

    case = _oracle_case(monkeypatch, f"loop{C}", _case_loop(C, P, k), 4, schur=True)
    (_, _, ci, pi, qs), (c0, p0), _, recs = case
    prob = ba.BAProblem(c0, p0, ci, pi, qs, tl_mode="flow", tile_mode=tiles, fixed=ba.FIXED_INTRINSICS)
    assert prob.lin_mode == lin
    S = prob._sched_host
    T, pt = int(S[1]), int(S[10])
    tasks = np.concatenate([S[S[pt + 2 * J]:S[pt + 2 * J] + 3 * S[pt + 2 * J + 1]]
                            for J in range(T)]).reshape(-1, 3)
    assert (tasks[:, 0] > 0).any()  # the reload path is taken
    assert not all(r[0] for r in recs)  # a rejected step is among the compared ones
    _compare(prob, case, 1e-8)


def _window10():
    cams, pts, ci, pi, qs = make_problem(7, 10, 800, 5)
    c0, p0 = _perturb(np.random.default_rng(8), cams, pts)
    return c0, p0, ci, pi, qs


@pytest.mark.gpu
def test_gpu_zero_mask_equals_no_mask():
    """An all-zero [C, 9] mask (the masked code path with nothing held) gives,
    bit for bit, the iterates of a problem built without the keyword."""
    from slam355 import ba

    w = _window10()
    a = ba.BAProblem(*w)
    b = ba.BAProblem(*w, fixed=np.zeros((10, 9), bool))
    assert a.fixed is None and b.fixed.tolist() == [0] * 10
    assert a._s.cam_fixed is None and b._s.cam_fixed
    a.iterate(4)
    b.iterate(4)
    assert a.state() == b.state()
    for x, y in zip(a.params(), b.params()):
        assert np.array_equal(x, y)


@pytest.mark.gpu
def test_gpu_fixed_in_batch_equals_solo():
    """A masked and an unmasked problem advanced by the same batched launches
    each equal their solo iterates bit for bit."""
    from slam355 import ba

    w0 = _window10()
    cams, pts, ci, pi, qs = make_problem(33, 6, 700, 4)
    w1 = (*_perturb(np.random.default_rng(133), cams, pts), ci, pi, qs)
    fx = np.tile(ba.FIXED_INTRINSICS, (10, 1))
    fx[0] = 1
    kw = [dict(fixed=fx), dict()]
    solo = [ba.BAProblem(*w, **k) for w, k in zip((w0, w1), kw)]
    for p in solo:
        p.iterate(4)
    batch = ba.BABatch([ba.BAProblem(*w, **k) for w, k in zip((w0, w1), kw)])
    batch.iterate(4)
    for a, b in zip(solo, batch.problems):
        assert a.state() == b.state()
        for x, y in zip(a.params(), b.params()):
            assert np.array_equal(x, y)
    assert np.array_equal(solo[0].params()[0][0], w0[0][0])  # the held camera did not move
    assert not np.array_equal(solo[1].params()[0][:, 6:], w1[0][:, 6:])  # the free intrinsics did


@pytest.mark.gpu
def test_gpu_window_set_fixed_equals_separate_problems():
    """BAWindowSet.build(fixed=) and .stage(fixed=) give every window the
    iterates BAProblem(fixed=) gives it alone, bit for bit (the equality of the
    unmasked window-set tests), for the windows the set builds itself and for
    the ones it hands to an ordinary slot-mode BAProblem; the held intrinsics
    keep their input bits and a later unmasked call is unmasked."""
    import torch
    from slam355 import ba

    inp, probs = stage_inputs(synthetic_windows([(800, 3), (300, 8), (1000, 2)], 8, 80), 8)
    s = torch.cuda.Stream()
    ws = ba.BAWindowSet()
    fx = np.tile(ba.FIXED_INTRINSICS, (8, 1))
    fx[0] = 1  # [n, 9]: the oldest keyframe of every window held whole
    refs = []
    for pr in probs:
        ref = ba.BAProblem(*pr, fixed=fx)
        ref.iterate(4)
        refs.append(ref.params())
    for how in ("build", "stage", "build"):
        got = ws.build(probs, s, fixed=fx) if how == "build" else ws.stage(*inp, stream=s, fixed=fx)
        assert [p.lin_mode for p in got] == ["mfma", "slot", "mfma"]
        assert all(np.array_equal(p.fixed, ba.fixed_mask(8, fx)) for p in got)
        with torch.cuda.stream(s):
            ba.BABatch([got[0], got[2]], stream=s).iterate(4)
            got[1].iterate(4)
        torch.cuda.synchronize()
        for w, (p, (rc, rp)) in enumerate(zip(got, refs)):
            gc, gp = p.params()
            assert np.array_equal(gc, rc) and np.array_equal(gp, rp), (how, w)
            assert np.array_equal(gc[:, 6:], probs[w][0][:, 6:]) and np.array_equal(gc[0], probs[w][0][0])
    # a [9] pattern over windows of different sizes; then no mask again
    mixed = [probs[0], (*_window10(),)]
    got = ws.build(mixed, s, fixed=ba.FIXED_INTRINSICS)
    plain = ws.build(mixed, s)
    with torch.cuda.stream(s):
        ba.BABatch(got, stream=s).iterate(3)
        ba.BABatch(plain, stream=s).iterate(3)
    torch.cuda.synchronize()
    for pr, g_, pl_ in zip(mixed, got, plain):
        for prob, kw in ((g_, dict(fixed=ba.FIXED_INTRINSICS)), (pl_, dict())):
            ref = ba.BAProblem(*pr, **kw)
            ref.iterate(3)
            for x, y in zip(ref.params(), prob.params()):
                assert np.array_equal(x, y)
    with pytest.raises(ValueError):
        ws.build(mixed, s, fixed=fx)  # [8, 9] does not fit the 10-camera window


@pytest.mark.gpu
def test_gpu_fixed_graph_replay_matches_eager():
    """iterate_graphed with a mask equals eager launches bit for bit."""
    from slam355 import ba

    w = _window10()
    fx = np.tile(ba.FIXED_INTRINSICS, (10, 1))
    fx[:2] = 1
    a = ba.BAProblem(*w, fixed=fx)
    b = ba.BAProblem(*w, fixed=fx)
    a.iterate(4)
    b.iterate_graphed(2)
    b.iterate_graphed(2)
    assert a.state() == b.state()
    for x, y in zip(a.params(), b.params()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.params()[0][:2], w[0][:2])


@pytest.mark.gpu
def test_gpu_bundle_adjustment_fixed_keyword():
    """The BundleAdjustment mirror passes `fixed` through: the solved cameras
    keep the held intrinsics' input bits, and the cost still drops."""
    from slam355 import BundleAdjustment as B
    from slam355 import ba

    cams, pts, ci, pi, qs = make_problem(3, 6, 150, 4)
    c0, p0 = _perturb(np.random.default_rng(4), cams, pts)
    r0, rf, x = B.bundle_adjustment(c0, p0, ci, pi, qs, fixed=ba.FIXED_INTRINSICS)
    assert np.array_equal(x[:54].reshape(6, 9)[:, 6:], c0[:, 6:])
    assert np.sum(rf ** 2) < 0.1 * np.sum(r0 ** 2)
    _, rf2, x2 = B.bundle_adjustment_with_sparsity(c0, p0, ci, pi, qs, None, fixed=ba.FIXED_INTRINSICS)
    assert np.array_equal(x2, x) and np.array_equal(rf2, rf)
