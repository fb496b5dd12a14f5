"""The tracking tail: F-LMedS as k_fm_solve / k_fm_score / k_fm_finish over a
candidate workspace, and PnP at the point counts where k_pnp changes path.

The F-LMedS split moves work between kernels and changes no arithmetic, so the
bar is the one the fused kernel met against the seeded CPU oracle: inlier mask
and count exact (test_geometry.py).  PnP: counts and masks exact and the pose
within 1e-8 (f64 LM on the same inlier set, reductions in another order).

Shapes: point counts on both sides of the 8-point minimum, of the 64-lane
wave, of the 768 errors a wave keeps in registers and, in a call of its own,
past the 1024 points a workgroup stages in LDS; hypothesis counts that leave
some of the 8 splits empty (< 8) and straddle k_fm_solve's 64-lane workgroup.
"""
import functools

import numpy as np
import pytest

from oracle import geometry as og

FM_CAP = 800
FM_COUNTS = (0, 7, 8, 9, 64, 65, 769, 800)  # 769 = 64 * 12 + 1
FM_NHYP = (1, 7, 63, 64, 65, 300)
FM_SEED, FM_ITEM0 = 9, 20
FM_BIG = 1100  # > 1024: k_fm_score reads the points from global memory
LDS_POINTS = 1024


def _stereo_points(seed, n, outliers=0.2):
    from slam355.synthetic import StereoRig

    rig = StereoRig(1280, 720)
    rng = np.random.default_rng(seed)
    Q = np.stack([rng.uniform(-15, 15, n), rng.uniform(-3, 3, n), rng.uniform(5, 80, n)], 1)
    pl = Q[:, :2] / Q[:, 2:3] * rig.K[0, 0] + rig.K[:2, 2] + rng.normal(0, 0.4, (n, 2))
    Qr = Q - [rig.baseline, 0, 0]
    pr = Qr[:, :2] / Qr[:, 2:3] * rig.K[0, 0] + rig.K[:2, 2] + rng.normal(0, 0.4, (n, 2))
    k = int(outliers * n)
    pr[:k] = rng.uniform([0, 0], [1280, 720], (k, 2))
    return pl, pr


@functools.lru_cache(maxsize=None)
def _fm_batch():
    """(m1, m2 [B, cap, 2], count) of the cap-800 batch; rows past count hold junk."""
    B = len(FM_COUNTS)
    rng = np.random.default_rng(77)
    m1 = rng.uniform(0, 700, (B, FM_CAP, 2))
    m2 = rng.uniform(0, 700, (B, FM_CAP, 2))
    for b, n in enumerate(FM_COUNTS):
        if n:
            m1[b, :n], m2[b, :n] = _stereo_points(30 + b, n)
    for a in (m1, m2):
        a.setflags(write=False)
    return m1, m2, np.array(FM_COUNTS, np.int32)


@functools.lru_cache(maxsize=None)
def _fm_big():
    a, c = _stereo_points(5, FM_BIG)
    return a[None].copy(), c[None].copy(), np.array([FM_BIG], np.int32)


@functools.lru_cache(maxsize=None)
def _fm_degenerate():
    """20 identical points; 20 collinear points shifted by (3, 0)."""
    m1 = np.zeros((2, 20, 2))
    m2 = np.zeros((2, 20, 2))
    m1[0] = m2[0] = [100.0, 50.0]
    m1[1] = np.stack([10.0 + 7.0 * np.arange(20), 20.0 + 3.5 * np.arange(20)], 1)
    m2[1] = m1[1] + [3.0, 0.0]
    return m1, m2, np.array([20, 20], np.int32)


@functools.lru_cache(maxsize=None)
def _fm_oracle(which, n_hyp, seed=FM_SEED, item0=FM_ITEM0):
    m1, m2, cnt = {"batch": _fm_batch, "big": _fm_big, "degenerate": _fm_degenerate}[which]()
    return [og.fundamental_lmeds(m1[b, :cnt[b]], m2[b, :cnt[b]], seed=seed, item=item0 + b,
                                 n_hyp=n_hyp)[:3] for b in range(len(cnt))]


def _T(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cached inputs stay read-only


def _check_fm(got, which, n_hyp, **kw):
    m1, m2, cnt = {"batch": _fm_batch, "big": _fm_big, "degenerate": _fm_degenerate}[which]()
    mask, F, n = (x.cpu().numpy() for x in got)
    for b, (em, eF, en) in enumerate(_fm_oracle(which, n_hyp, **kw)):
        assert n[b] == en, (which, n_hyp, b, int(n[b]), en)
        assert np.array_equal(mask[b, :cnt[b]].astype(bool), em), (which, n_hyp, b)
        if en < 0:
            assert not mask[b, :cnt[b]].any() and np.all(F[b] == 0.0), (which, n_hyp, b)


# ----------------------------------------------------------------------------- CPU
def test_oracle_degenerate_pairs_have_no_model():
    for em, eF, en in _fm_oracle("degenerate", 300):
        assert en == -1 and not em.any() and np.all(eF == 0.0)


def test_fundamental_workspace_errors_without_gpu():
    """A workspace one double short: status -1 and the needed length, before any GPU call."""
    from slam355 import _lib

    need = _lib.lib.slam_fundamental_workspace_len(4, 300)
    assert need >= 4 * 300 * 28
    rc = _lib.lib.slam_fundamental_lmeds_ws(None, None, None, 800, 4, 0, 0, 300, None, None, None,
                                            None, need - 1, None)
    assert rc == -1 and str(need).encode() in _lib.lib.slam_last_error()
    # with enough workspace the next check (null pointers) is reached, still without a GPU
    rc = _lib.lib.slam_fundamental_lmeds_ws(None, None, None, 800, 4, 0, 0, 300, None, None, None,
                                            None, need, None)
    assert rc == -1 and b"null" in _lib.lib.slam_last_error()


def test_fundamental_workspace_len_monotone():
    from slam355 import _lib

    f = _lib.lib.slam_fundamental_workspace_len
    sizes = (0, 1, 2, 7, 64, 65, 300, 4096)
    for b in sizes:
        row = [f(b, h) for h in sizes]
        col = [f(h, b) for h in sizes]
        assert row == sorted(row) and col == sorted(col) and min(row) >= 0
    assert f(1 << 20, 4096) == (1 << 20) * 4096 * 28  # no 32-bit overflow


# ----------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n_hyp", FM_NHYP)
def test_gpu_fm_split_matches_oracle(n_hyp):
    """Counts around the 8-point minimum, the wave and the register-cached 768;
    n_hyp < 8 leaves splits empty; both entry points agree bit for bit."""
    from slam355 import geometry

    m1, m2, cnt = _fm_batch()
    t1, t2, tc = _T(m1), _T(m2), _T(cnt)
    ws = geometry.fundamental_workspace(len(cnt), n_hyp)
    got = geometry.fundamental_lmeds(t1, t2, tc, seed=FM_SEED, item0=FM_ITEM0, n_hyp=n_hyp, ws=ws)
    _check_fm(got, "batch", n_hyp)
    plain = geometry.fundamental_lmeds(t1, t2, tc, seed=FM_SEED, item0=FM_ITEM0, n_hyp=n_hyp)
    for a, c in zip(got, plain):
        a, c = a.cpu().numpy(), c.cpu().numpy()
        assert np.array_equal(a.view(np.uint8), c.view(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("n_hyp", FM_NHYP)
def test_gpu_fm_split_points_past_lds(n_hyp):
    """One pair with more points than a workgroup stages in LDS."""
    from slam355 import geometry

    m1, m2, cnt = _fm_big()
    assert cnt[0] > LDS_POINTS
    ws = geometry.fundamental_workspace(1, n_hyp)
    got = geometry.fundamental_lmeds(_T(m1), _T(m2), _T(cnt), seed=FM_SEED, item0=FM_ITEM0,
                                     n_hyp=n_hyp, ws=ws)
    _check_fm(got, "big", n_hyp)


@pytest.mark.gpu
def test_gpu_fm_split_degenerate_pairs():
    from slam355 import geometry

    m1, m2, cnt = _fm_degenerate()
    got = geometry.fundamental_lmeds(_T(m1), _T(m2), _T(cnt), seed=FM_SEED, item0=FM_ITEM0,
                                     ws=geometry.fundamental_workspace(2, 300))
    _check_fm(got, "degenerate", 300)
    assert np.all(got[2].cpu().numpy() == -1)


@pytest.mark.gpu
def test_gpu_fm_workspace_reuse_reads_no_stale_records():
    """n_hyp = 300 then n_hyp = 7 on the same workspace and stream."""
    from slam355 import geometry

    m1, m2, cnt = _fm_batch()
    t1, t2, tc = _T(m1), _T(m2), _T(cnt)
    ws = geometry.fundamental_workspace(len(cnt), 300)
    first = geometry.fundamental_lmeds(t1, t2, tc, seed=FM_SEED, item0=FM_ITEM0, n_hyp=300, ws=ws)
    _check_fm(first, "batch", 300)
    second = geometry.fundamental_lmeds(t1, t2, tc, seed=FM_SEED, item0=FM_ITEM0, n_hyp=7, ws=ws)
    _check_fm(second, "batch", 7)


@pytest.mark.gpu
def test_gpu_fm_short_workspace_is_refused():
    from slam355 import _lib, geometry

    m1, m2, cnt = _fm_degenerate()
    ws = geometry.fundamental_workspace(2, 300)
    with pytest.raises(_lib.SlamError, match=str(2 * 300 * 28)):
        geometry.fundamental_lmeds(_T(m1), _T(m2), _T(cnt), n_hyp=300, ws=ws[:-1])


PNP_COUNTS = (4, 5, 6, 150, 64 * 4 + 1)  # 64 kRc + 1: one point past the register-cached ones
PNP_NHYP = (1, 100, 256)
PNP_SEED, PNP_ITEM0 = 11, 100


@functools.lru_cache(maxsize=None)
def _pnp_batch():
    from slam355.synthetic import StereoRig

    K = StereoRig(1280, 720).K
    B, cap = len(PNP_COUNTS), max(PNP_COUNTS)
    rng = np.random.default_rng(3)
    Q = rng.uniform(1, 50, (B, cap, 3))
    q = rng.uniform(0, 700, (B, cap, 2))
    for b, n in enumerate(PNP_COUNTS):
        X = np.stack([rng.uniform(-10, 10, n), rng.uniform(-3, 3, n), rng.uniform(5, 60, n)], 1)
        r = np.array([0.002, 0.01, -0.003]) * (1 + b)
        Xc = X @ og.rodrigues(r).T + [0.02, -0.01, -1.0]
        uv = Xc[:, :2] / Xc[:, 2:3] * K[0, 0] + K[:2, 2] + rng.normal(0, 0.5, (n, 2))
        k = int(0.2 * n) if n > 6 else 0  # 5 or 6 points: no outliers, a 5-point sample is all there is
        uv[:k] += rng.uniform(-120, 120, (k, 2))
        Q[b, :n], q[b, :n] = X, uv
    return Q, q, np.array(PNP_COUNTS, np.int32), K


@functools.lru_cache(maxsize=None)
def _pnp_oracle(n_hyp):
    Q, q, cnt, K = _pnp_batch()
    return [og.pnp_ransac(Q[b, :cnt[b]], q[b, :cnt[b]], K, seed=PNP_SEED, item=PNP_ITEM0 + b,
                          n_hyp=n_hyp) for b in range(len(cnt))]


@pytest.mark.gpu
@pytest.mark.parametrize("n_hyp", PNP_NHYP)
def test_gpu_pnp_edge_counts_match_oracle(n_hyp):
    """The L < 5 guard, a sample that is all the points, and one point past the
    64 kRc a refining lane keeps in registers; 1, the default and the most hypotheses."""
    from slam355 import geometry

    Q, q, cnt, K = _pnp_batch()
    rv, tv, n, mask = (x.cpu().numpy() for x in geometry.pnp_ransac(
        _T(Q), _T(q), _T(cnt), K, seed=PNP_SEED, item0=PNP_ITEM0, n_hyp=n_hyp))
    for b, (erv, etv, en, emask) in enumerate(_pnp_oracle(n_hyp)):
        L = cnt[b]
        assert n[b] == en, (n_hyp, b, int(n[b]), en)
        if en < 0:  # the L < 5 guard
            assert L < 5 and np.all(rv[b] == 0) and np.all(tv[b] == 0) and not mask[b, :L].any()
            continue
        assert np.array_equal(mask[b, :L].astype(bool), emask), (n_hyp, b)
        print(f"n_hyp {n_hyp} L {L}: |drvec| {np.abs(rv[b] - erv).max():.2e} "
              f"|dtvec| {np.abs(tv[b] - etv).max():.2e}")
        assert np.allclose(rv[b], erv, rtol=0, atol=1e-8), (n_hyp, b)
        assert np.allclose(tv[b], etv, atol=1e-8), (n_hyp, b)
