"""k_pnp_hyp_eig's group mapping (five hypotheses a wave on 12 lanes each, four
lanes idle) at hypothesis counts that fill its waves differently.

Sample h of an item depends only on (seed, item, h), so the poses of a call
with n_hyp = n are the first n of the call with n_hyp = 100: no new golden file,
the prefix of tests/golden/pnp_hyp_golden.npz (test_pnp_split.py describes its
five items) is the expectation, bit for bit, NaN positions and signs included.

n_hyp 5 fills one wave, 4 leaves one group dead, 7 is a full wave + 2, 11 two
full waves + 1, 99 leaves the last wave short by one.  A dead group, and every
group of the guarded item (count 4), writes nothing: those workspace rows keep
their NaN fill.
"""
import functools
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_hyp_golden.npz")
N_HYP = (5, 4, 7, 11, 99)
SEED, ITEM0 = 21, 300  # tests/golden/make_pnp_hyp_goldens.py
GUARD = 2              # the item with count 4


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


def _buffers(n_hyp, caller_scratch, extra=0):
    """(ws of n_hyp + extra hypotheses per item filled with NaN, scratch or None, outputs)."""
    import torch
    from slam355 import geometry

    B, cap = _golden()["Q"].shape[:2]
    ws = torch.full((B * (n_hyp + extra) * 6,), float("nan"), dtype=torch.float64, device="cuda")
    scratch = geometry.pnp_scratch(B, n_hyp) if caller_scratch else None
    out = tuple(torch.zeros(s, dtype=t, device="cuda") for s, t in
                (((B, 3), torch.float64), ((B, 3), torch.float64), ((B,), torch.int32),
                 ((B, cap), torch.uint8)))
    return ws, scratch, out


def _launch(n_hyp, hyp_iters, bufs, stream=None):
    from slam355 import geometry

    Q, q, cnt = _inputs()
    ws, scratch, out = bufs
    geometry.pnp_ransac(Q, q, cnt, _golden()["K"], seed=SEED, item0=ITEM0, n_hyp=n_hyp,
                        hyp_iters=hyp_iters, ws=ws, scratch=scratch, out=out, stream=stream)
    return ws


def _same_bits(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    assert np.array_equal(got, exp, equal_nan=True), what + (int((got != exp).sum()),)
    assert np.array_equal(np.isnan(got), np.isnan(exp)) and np.array_equal(
        np.signbit(got), np.signbit(exp)), what


def _check_prefix(ws, n_hyp, hyp_iters, extra=0):
    """ws [B][n_hyp][6] (+ extra untouched rows behind it) against the first
    n_hyp hypotheses of the n_hyp = 100 golden."""
    g = _golden()
    B = len(g["count"])
    name = "ws0_100" if hyp_iters == 0 else "ws10_100"
    exp = np.ascontiguousarray(g[name].reshape(B, 100, 6)[:, :n_hyp])
    got = ws.cpu().numpy()
    body = got[:B * n_hyp * 6].reshape(B, n_hyp, 6)
    _same_bits(body, exp, (name, n_hyp))
    assert np.isnan(body[GUARD]).all(), (name, n_hyp, "guarded item written")
    assert np.isnan(got[B * n_hyp * 6:]).all(), (name, n_hyp, "rows past n_hyp written")


@pytest.mark.gpu
@pytest.mark.parametrize("caller_scratch", (True, False), ids=("caller_scratch", "pool_scratch"))
@pytest.mark.parametrize("n_hyp", N_HYP)
def test_gpu_pnp_hypothesis_prefix_equals_golden(n_hyp, caller_scratch):
    """EPnP poses (hyp_iters=0) and sample-LM poses (hyp_iters=10) of n_hyp = n
    equal the first n of the n_hyp = 100 golden; the rows of hypotheses >= n_hyp
    (the workspace is one hypothesis per item longer than the call needs) and of
    the guarded item stay NaN."""
    import torch

    g = _golden()
    assert int(g["count"][GUARD]) == 4 and np.isnan(g["ws0_100"].reshape(5, -1)[GUARD]).all()
    for hyp_iters in (0, 10):
        ws = _launch(n_hyp, hyp_iters, _buffers(n_hyp, caller_scratch, extra=1))
        torch.cuda.synchronize()
        _check_prefix(ws, n_hyp, hyp_iters, extra=1)


@pytest.mark.gpu
def test_gpu_pnp_dead_groups_leave_the_scratch_alone():
    """The eigen kernel's record of a hypothesis >= n_hyp does not exist: a
    caller scratch one record per item longer than slam_pnp_scratch_len keeps
    its NaN fill there, at n_hyp 4 (a dead group in the only wave) and 7."""
    import torch
    from slam355 import _lib

    B = len(_golden()["count"])
    for n_hyp in (4, 7):
        need = int(_lib.lib.slam_pnp_scratch_len(B, n_hyp))
        ws, _, out = _buffers(n_hyp, False)
        scratch = torch.full((need + B * 106,), float("nan"), dtype=torch.float64, device="cuda")
        _launch(n_hyp, 0, (ws, scratch, out))
        torch.cuda.synchronize()
        assert torch.isnan(scratch[need:]).all(), n_hyp
        rec = scratch[:need].reshape(B, n_hyp, 106)
        assert torch.isnan(rec[GUARD]).all(), n_hyp          # the guarded item: no record
        flags = rec[[i for i in range(B) if i != GUARD], :, 0]
        assert bool(((flags == 0) | (flags == 1)).all()), n_hyp  # every live group wrote its flag
        _check_prefix(ws, n_hyp, 0)


@pytest.mark.gpu
def test_gpu_pnp_two_streams_short_waves():
    """Two calls that may overlap, n_hyp 7 and 99, each with its own workspace
    and scratch: both give what they give alone."""
    import torch

    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    # every buffer exists, and stays referenced, from before the first launch to
    # after the last kernel: the caching allocator hands none of them out twice
    b1, b2, b3 = _buffers(7, True), _buffers(99, True), _buffers(7, False)
    _inputs()
    torch.cuda.synchronize()  # the fills above ran on the current stream
    r1 = _launch(7, 10, b1, stream=s1)
    r2 = _launch(99, 10, b2, stream=s2)
    r3 = _launch(7, 10, b3, stream=s1)  # pool scratch, ordered on its stream
    torch.cuda.synchronize()
    _check_prefix(r1, 7, 10)
    _check_prefix(r2, 99, 10)
    _check_prefix(r3, 7, 10)
