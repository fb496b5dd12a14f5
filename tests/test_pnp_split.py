"""The PnP hypothesis chain (k_pnp_hyp_eig -> k_pnp_hyp_beta -> k_pnp_hyp_lm)
pinned bit for bit to the fused k_pnp_hyp (+ k_pnp_hyp_lm) it replaced:
tests/golden/pnp_hyp_golden.npz holds what that commit computed
(tests/golden/make_pnp_hyp_goldens.py, which also describes the five items).
The split moves work between kernels and lanes and changes no arithmetic, so
every comparison is np.array_equal, NaN positions included: the EPnP poses
(hyp_iters=0), the poses after the sample LM, and rvec, tvec, ninliers, mask.

Shapes: the smallest at which each kernel can go wrong -- counts 5 (the
minimum), 37, 4 (the guard), 12 coincident points (every sample degenerate) and
48 with a large rotation, rows past each count NaN; n_hyp 100 (the default),
6 (no multiple of 4 or 16: the last workgroup of each kernel holds dead
groups, k_pnp_hyp_beta runs one partly filled wave) and 1.
"""
import functools
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_hyp_golden.npz")
N_HYP = (100, 6, 1)
SEED, ITEM0 = 21, 300  # make_pnp_hyp_goldens.py


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    for a in g.values():
        a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _inputs():
    """The golden inputs on the device (shared, never written)."""
    import torch

    g = _golden()
    return tuple(torch.from_numpy(np.array(g[k])).cuda() for k in ("Q", "q", "count"))


def _buffers(n_hyp, caller_scratch):
    """(ws filled with NaN, scratch or None, (rvec, tvec, ninliers, mask)) for one call."""
    import torch
    from slam355 import geometry

    B, cap = _golden()["Q"].shape[:2]
    ws = torch.full((B * n_hyp * 6,), float("nan"), dtype=torch.float64, device="cuda")
    scratch = geometry.pnp_scratch(B, n_hyp) if caller_scratch else None
    out = tuple(torch.zeros(s, dtype=t, device="cuda") for s, t in
                (((B, 3), torch.float64), ((B, 3), torch.float64), ((B,), torch.int32),
                 ((B, cap), torch.uint8)))
    return ws, scratch, out


def _launch(n_hyp, hyp_iters, bufs, stream=None):
    """One pnp_ransac call -> (ws, rvec, tvec, ninliers, mask) tensors."""
    from slam355 import geometry

    Q, q, cnt = _inputs()
    ws, scratch, out = bufs
    geometry.pnp_ransac(Q, q, cnt, _golden()["K"], seed=SEED, item0=ITEM0, n_hyp=n_hyp,
                        hyp_iters=hyp_iters, ws=ws, scratch=scratch, out=out, stream=stream)
    return (ws,) + out


def _same(got, name, n_hyp):
    exp = _golden()[f"{name}_{n_hyp}"]
    got = got.cpu().numpy()
    assert got.dtype == exp.dtype and got.shape == exp.shape, (name, n_hyp)
    assert np.array_equal(got, exp, equal_nan=True), (name, n_hyp, int((got != exp).sum()))
    if got.dtype == np.float64:  # the same bits, not only the same values
        assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(
            np.signbit(got), np.signbit(exp)), (name, n_hyp)


def _check(res, n_hyp, hyp_iters):
    if hyp_iters == 0:
        _same(res[0], "ws0", n_hyp)
        return
    for got, name in zip(res, ("ws10", "rvec", "tvec", "ninliers", "mask")):
        _same(got, name, n_hyp)


@pytest.mark.gpu
@pytest.mark.parametrize("caller_scratch", (True, False), ids=("caller_scratch", "pool_scratch"))
@pytest.mark.parametrize("n_hyp", N_HYP)
def test_gpu_pnp_hypotheses_equal_fused_kernel(n_hyp, caller_scratch):
    """slam_pnp_ransac_ws (caller scratch) and slam_pnp_ransac (pool scratch): the
    EPnP poses, the LM poses and the final result equal the fused kernel's."""
    import torch

    g = _golden()
    assert int(g["ninliers_100"][2]) == -1 and np.isnan(g["ws0_100"].reshape(5, -1)[2]).all()
    assert (g["ws0_100"].reshape(5, 100, 6)[3] == 0).all()  # coincident: every EPnP fails
    for hyp_iters in (0, 10):
        res = _launch(n_hyp, hyp_iters, _buffers(n_hyp, caller_scratch))
        torch.cuda.synchronize()
        _check(res, n_hyp, hyp_iters)


@pytest.mark.gpu
def test_gpu_pnp_short_scratch_is_refused_before_any_launch():
    import torch
    from slam355 import _lib, geometry

    g = _golden()
    Q, q, cnt = _inputs()
    B, n_hyp = len(g["count"]), 6
    need = int(_lib.lib.slam_pnp_scratch_len(B, n_hyp))
    assert need == B * n_hyp * 106 and geometry.pnp_scratch(B, n_hyp).numel() == need
    assert int(_lib.lib.slam_pnp_workspace_len(B, n_hyp)) == B * n_hyp * 6
    ws = torch.full((B * n_hyp * 6,), float("nan"), dtype=torch.float64, device="cuda")
    out = (torch.full((B, 3), 7.0, dtype=torch.float64, device="cuda"),
           torch.full((B, 3), 7.0, dtype=torch.float64, device="cuda"),
           torch.full((B,), 7, dtype=torch.int32, device="cuda"),
           torch.full((B, Q.shape[1]), 7, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.SlamError, match=str(need)) as e:
        geometry.pnp_ransac(Q, q, cnt, g["K"], seed=SEED, item0=ITEM0, n_hyp=n_hyp, ws=ws,
                            out=out, scratch=geometry.pnp_scratch(B, n_hyp)[:-1])
    assert "(-3)" in str(e.value) and "scratch" in str(e.value)  # SLAM_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert torch.isnan(ws).all() and all(bool((o == 7).all()) for o in out)


@pytest.mark.gpu
def test_gpu_pnp_two_streams_with_own_buffers():
    """Two calls that may overlap, each with its own workspace and scratch: both
    give what they give one after the other (the goldens)."""
    import torch

    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    # every buffer exists, and stays referenced, from before the first launch to
    # after the last kernel: the caching allocator hands none of them out twice
    b1, b2, b3 = _buffers(100, True), _buffers(6, True), _buffers(100, False)
    _inputs()
    torch.cuda.synchronize()  # the fills above ran on the current stream
    r1 = _launch(100, 10, b1, stream=s1)
    r2 = _launch(6, 10, b2, stream=s2)
    r3 = _launch(100, 10, b3, stream=s2)  # pool scratch, ordered on its stream
    torch.cuda.synchronize()
    _check(r1, 100, 10)
    _check(r2, 6, 10)
    _check(r3, 100, 10)
