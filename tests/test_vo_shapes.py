"""Stereo-VO pose kernels beyond test_vo.py's one batch: k_vo_err past its
first chunk of 8192 norms (and its 64 KiB of dynamic LDS), the limits of
max_iter / early_stop / lm_iters, and the batched residual entry with ragged
counts.  Scenes and bars are test_vo.py's.
"""
import numpy as np
import pytest

import shapes_ref as sr
from oracle import geometry as og
from test_vo import P_L, _scene

# 2N = 8192 fills the first chunk exactly, 8194 spills two norms, 16400 takes three chunks
LARGE_NS = [4096, 4097, 8200, 0, 5]
# the seed is chosen so that the CPU test below holds for every item: with 5 points two
# hypotheses can draw the same 6-sample in another order (errors one ulp apart, as
# seed 9 does), and with this one the chosen hypotheses are 4, 7, 4 and 9, not 0
LARGE_SEED, LARGE_ITEM0 = 15, 4

PARAM_CASES = [dict(max_iter=1), dict(max_iter=128), dict(max_iter=128, early_stop=128),
               dict(early_stop=1), dict(lm_iters=0)]
PARAM_SEED, PARAM_ITEM = 9, 4


@pytest.fixture(scope="module")
def large():
    """The batch (consecutive _scene calls of default_rng(1)) and the oracle's result per item."""
    rng = np.random.default_rng(1)
    cap = max(LARGE_NS)
    A = [np.zeros((len(LARGE_NS), cap, k)) for k in (2, 2, 3, 3)]
    for b, n in enumerate(LARGE_NS):
        if n:
            for a, v in zip(A, _scene(rng, n)[:4]):
                a[b, :n] = v
    want = [og.vo_estimate_pose(*(a[b, :n] for a in A), P_L, seed=LARGE_SEED, item=LARGE_ITEM0 + b)
            for b, n in enumerate(LARGE_NS)]
    return A, want


@pytest.fixture(scope="module")
def scene150():
    """With seed 9, item 4 the defaults choose hypothesis 8 of 14 tried here and
    max_iter = early_stop = 128 chooses 125: the top of the hypothesis range counts."""
    return _scene(np.random.default_rng(8), 150)[:4]


def _oracle150(scene150, kw):
    return og.vo_estimate_pose(*scene150, P_L, seed=PARAM_SEED, item=PARAM_ITEM, **kw)


# ----------------------------------------------------------------------------- CPU
def test_oracle_selection_cannot_flip_on_rounding(large):
    """The 1e-9 error bar leaves the selection alone only if no two distinct
    errors the sequential loop compared are that close: demand 1e-6."""
    _, want = large
    for n, (_, best, ntried, err, errs) in zip(LARGE_NS, want):
        if n == 0:
            assert best == -1 and ntried == 0
            continue
        assert ntried >= 6 and err == errs[best]
        gap = sr.distinct_rel_gap(errs[:ntried])
        print(f"n = {n}: best {best}, ntried {ntried}, smallest distinct gap {gap:.3g}")
        assert gap >= 1e-6, (n, gap)


@pytest.mark.parametrize("kw", PARAM_CASES, ids=str)
def test_oracle_parameter_cases(scene150, kw):
    dof, best, ntried, err, errs = _oracle150(scene150, kw)
    mi, es = kw.get("max_iter", 100), kw.get("early_stop", 5)
    assert 0 <= best < ntried <= mi
    if kw == dict(max_iter=128, early_stop=128):
        assert ntried == 128  # the loop cannot stop early: every hypothesis is tried
    if kw == dict(early_stop=1):
        assert ntried == best + 2  # the first hypothesis that does not improve ends the loop
    if kw == dict(lm_iters=0):
        # no LM step: every hypothesis is dof = 0, every error the same number
        assert len(set(errs[:ntried])) == 1 and best == 0 and ntried == es + 1
        assert not np.any(dof)
    else:
        assert sr.distinct_rel_gap(errs[:ntried]) >= 1e-6


# ----------------------------------------------------------------------------- GPU
def _gpu_pose(A, ns, seed, item0, **kw):
    import torch
    from slam355 import geometry

    dev = torch.device("cuda")
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in A]
    cnt = torch.tensor(ns, dtype=torch.int32, device=dev)
    out = geometry.vo_estimate_pose(*t, cnt, P_L, seed=seed, item0=item0, **kw)
    return [x.cpu().numpy() for x in out]


@pytest.mark.gpu
def test_gpu_vo_pose_beyond_one_error_chunk(large):
    A, want = large
    pose, best, ntried, err = _gpu_pose(A, LARGE_NS, LARGE_SEED, LARGE_ITEM0)
    for b, n in enumerate(LARGE_NS):
        d, bo, nt, eo, _ = want[b]
        assert best[b] == bo and ntried[b] == nt, b
        assert np.allclose(pose[b], d, rtol=1e-8, atol=1e-10), b
        if n:
            assert abs(err[b] - eo) <= 1e-9 * eo, b


@pytest.mark.gpu
@pytest.mark.parametrize("kw", PARAM_CASES, ids=str)
def test_gpu_vo_pose_parameter_limits(scene150, kw):
    d, bo, nt, eo, _ = _oracle150(scene150, kw)
    pose, best, ntried, err = _gpu_pose([a[None] for a in scene150], [150], PARAM_SEED, PARAM_ITEM,
                                        **kw)
    assert best[0] == bo and ntried[0] == nt
    assert np.allclose(pose[0], d, rtol=1e-8, atol=1e-10)
    assert abs(err[0] - eo) <= 1e-9 * eo
    if kw == dict(lm_iters=0):
        assert best[0] == 0 and ntried[0] == 6 and not np.any(pose[0])


@pytest.mark.gpu
@pytest.mark.parametrize("max_iter", [0, 129])
def test_gpu_vo_pose_refuses_max_iter_outside_1_128(scene150, max_iter):
    from slam355 import _lib

    with pytest.raises(_lib.SlamError):
        _gpu_pose([a[None] for a in scene150], [150], PARAM_SEED, PARAM_ITEM, max_iter=max_iter)


@pytest.mark.gpu
def test_gpu_vo_residuals_batched_ragged():
    """B = 3, cap = 321 (4 cap = 1284 is no multiple of the workgroup), counts
    [321, 0, 77]: item b's first 4 count[b] entries in the reference's flat
    order for ITS count, the rest of the row untouched."""
    import torch
    from slam355 import geometry

    rng = np.random.default_rng(12)
    cap, ns = 321, [321, 0, 77]
    A = [np.zeros((3, cap, k)) for k in (2, 2, 3, 3)]
    dofs = np.zeros((3, 6))
    for b in range(3):
        *v, dof = _scene(rng, cap)  # every row holds data: rows past count must be ignored
        for a, x in zip(A, v):
            a[b] = x
        dofs[b] = dof
    dofs[1] *= 3.0
    dofs[2] = 0.0
    dev = torch.device("cuda")
    t = [torch.from_numpy(a).to(dev) for a in A]
    out = torch.full((3, 4 * cap), float("nan"), dtype=torch.float64, device=dev)
    f = geometry.vo_residuals(torch.from_numpy(dofs).to(dev), *t,
                              torch.tensor(ns, dtype=torch.int32, device=dev), P_L, out=out)
    assert f is out
    f = f.cpu().numpy()
    for b, n in enumerate(ns):
        ref = og.vo_residuals(dofs[b], *(a[b, :n] for a in A), P_L)
        assert ref.shape == (4 * n,)
        assert np.allclose(f[b, :4 * n], ref, rtol=1e-9, atol=1e-9), b
        assert np.all(np.isnan(f[b, 4 * n:])), b
