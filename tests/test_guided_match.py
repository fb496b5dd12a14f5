"""Guided matching (search by projection): slam_project_landmarks, slam_kp_grid,
slam_hamming_window_knn2, slam_match_unique, slam_track_rows and LandmarkMap.

The bar is bit-exact against tests/guided_ref.py (a NumPy restatement of the
header's definitions), which is itself pinned to the exact kNN-2 oracle; the
projection is held to 1 f32 ulp with an identical valid pattern.
"""
import numpy as np
import pytest

import guided_ref as gr
import oracle

W, H = 160, 96
SETTINGS = [(256, (7, 10)), (64, (9, 10)), (0, (1, 1))]
RADII = [0.5, 7.0, 20.0, 200.0]
EDGE_R = [0.5, 7.0, 20.0]   # the radii of the queries with a keypoint exactly on the window edge


def _flip(rng, d, nbits):
    bits = np.unpackbits(d, axis=-1)
    for row in bits.reshape(-1, 256):
        row[rng.choice(256, nbits, replace=False)] ^= 1
    return np.packbits(bits, axis=-1)


def _desc_sets(rng, nq=203, nt=300):
    """Random targets with one duplicated block (ties), queries near some of them."""
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    t[40:60] = t[100:120]
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    src = rng.integers(0, nt, nq)
    near = rng.random(nq) < 0.6
    q[near] = _flip(rng, t[src[near]], 12)
    q[:10] = t[100:110]          # exact copies of duplicated rows: distance-0 ties
    return q, t


# ----------------------------------------------------------------------------- CPU
def test_ref_equals_knn2_oracle_without_window():
    rng = np.random.default_rng(11)
    q, t = _desc_sets(rng)
    kp = np.zeros((300, 5), np.float32)
    kp[:, 0], kp[:, 1] = rng.uniform(0, W - 1, 300), rng.uniform(0, H - 1, 300)
    quv = np.stack([rng.uniform(0, W, 203), rng.uniform(0, H, 203)], 1).astype(np.float32)
    qr = np.full(203, np.inf, np.float32)
    for nt in (300, 2, 1, 0):
        i2, d2, g = gr.window_knn2(q, quv, qr, t, kp, nt, W, H, 256, (7, 10))
        ei2, ed2, eg = oracle.hamming_knn2(q, t[:nt])
        assert np.array_equal(i2, ei2) and np.array_equal(d2, ed2)
        if nt >= 2:
            assert np.array_equal(g.astype(bool), np.asarray(eg).astype(bool))
        elif nt == 1:
            assert g.all()       # one candidate is enough here (d1 <= 256 always)
    assert (d2[:10, 0] == -1).all() and (ed2[:10, 0] == -1).all()  # nt = 0 came last
    i2, d2, _ = gr.window_knn2(q, quv, qr, t, kp, 300, W, H, 256, (7, 10))
    assert (d2[:10] == 0).all() and (i2[:10, 0] < i2[:10, 1]).all()  # ties -> lower index first


def test_argument_errors_without_gpu():
    from slam355 import _lib

    L = _lib.lib
    err = lambda: L.slam_last_error()  # noqa: E731
    N = None
    # slam_project_landmarks
    assert L.slam_project_landmarks(N, 1, N, 10, 1, N, N, W, H, 0.0, 0.1, N, N, N) == -1
    assert b"null" in err()
    assert L.slam_project_landmarks(N, 1, N, 10, 1, N, N, W, H, -1.0, 0.1, N, N, N) == -1
    assert b"margin" in err()
    # slam_kp_grid
    assert L.slam_kp_grid(N, N, 10, 1, W, H, 32, N, N, N) == -1 and b"null" in err()
    assert L.slam_kp_grid(N, N, 10, 1, W, H, 24, N, N, N) == -1 and b"cell" in err()
    assert L.slam_kp_grid(N, N, 70000, 1, W, H, 32, N, N, N) == -1 and b"kp_cap" in err()
    assert L.slam_kp_grid(N, N, 10, 1, 16 * 129, 16 * 128, 16, N, N, N) == -1 and b"cells" in err()
    # slam_hamming_window_knn2
    def knn(q_cap=10, t_cap=10, w=W, h=H, cell=32, md=64, num=7, den=10):
        return L.slam_hamming_window_knn2(N, 1, N, N, N, q_cap, N, N, N, t_cap, N, N, w, h, cell, 1,
                                          md, num, den, N, N, N, N)
    assert knn() == -1 and b"null" in err()
    assert knn(cell=24) == -1 and b"cell" in err()
    assert knn(t_cap=70000) == -1 and b"t_cap" in err()
    assert knn(q_cap=(1 << 20) + 1) == -1 and b"q_cap" in err()
    assert knn(den=0) == -1 and b"ratio" in err()
    assert knn(num=11) == -1 and b"ratio" in err()
    assert knn(md=300) == -1 and b"max_dist" in err()
    assert knn(w=16 * 129, h=16 * 128, cell=16) == -1 and b"cells" in err()
    # slam_match_unique
    assert L.slam_match_unique(N, N, N, N, 10, 10, 1, N, N, N) == -1 and b"null" in err()
    assert L.slam_match_unique(N, N, N, N, 10, 70000, 1, N, N, N) == -1 and b"t_cap" in err()
    # slam_track_rows
    assert L.slam_track_rows(N, N, N, 10, N, 12, 1, 0, 10, N, N, N) == -1 and b"null" in err()
    assert L.slam_track_rows(N, N, N, 10, N, 12, 1, 0, 9, N, N, N) == -1 and b"rows_cap" in err()


# ----------------------------------------------------------------------------- GPU
def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pile(rng, n):
    """n keypoints inside the one cell [32, 48)^2 (for cell 16 and, with it, 32)."""
    return np.stack([rng.uniform(33, 47, n), rng.uniform(33, 47, n)], 1).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("cell,size", [pytest.param(16, (W, H), id="16"), pytest.param(32, (W, H), id="32"),
                                       pytest.param(16, (640, 480), id="16-640x480")])
def test_kp_grid(cell, size):
    """160 x 96: 60 or 15 cells, fewer than the workgroup's 1024 lanes; 640 x 480 at
    cell 16: 1200 cells, two per lane of the scan."""
    from slam355 import matcher

    W, H = size
    rng = np.random.default_rng(5)
    cap = 300
    kp = np.zeros((3, cap, 5), np.float32)
    kp[..., 0] = rng.uniform(0, W, (3, cap))
    kp[..., 1] = rng.uniform(0, H, (3, cap))
    kp[..., 2:] = rng.uniform(0, 1, (3, cap, 3))
    k = kp[2]
    k[:90, :2] = _pile(rng, 90)
    k[90, 0] = 0.0
    k[91, 0] = np.nextafter(np.float32(W), np.float32(0))
    k[92, 0] = W                       # outside
    k[93, 1] = np.nextafter(np.float32(H), np.float32(0))
    k[94, 1] = H                       # outside
    k[95, 0] = -0.25                   # outside
    k[96, 1] = -3.0                    # outside
    k[97, 0] = np.nan                  # outside
    k[98, 1] = np.nan                  # outside
    k[99, :2] = (0.0, 0.0)
    n = np.array([0, 1, cap], np.int32)
    g = matcher.KeypointGrid(_dev(kp), _dev(n), W, H, cell)
    cp, ck = g.cell_ptr.cpu().numpy(), g.cell_kp.cpu().numpy()
    for b in range(3):
        ep, members = gr.kp_grid(kp[b], n[b], W, H, cell)
        assert np.array_equal(cp[b], ep), b
        for c, m in enumerate(members):
            assert np.array_equal(np.sort(ck[b, ep[c]:ep[c + 1]]), m), (b, c)
    ep, members = gr.kp_grid(kp[2], cap, W, H, cell)
    assert ep[-1] == cap - 6 and max(len(m) for m in members) >= 90
    # ORB's overflow code (a negative count) is an empty set
    g.build(_dev(kp), _dev(np.array([-1, -7, 2], np.int32)))
    cp = g.cell_ptr.cpu().numpy()
    assert (cp[:2] == 0).all() and cp[2, -1] == 2


def _search_scene(radius):
    """Batch 3: (nq, nt) = (0, 0), (1, 1), (203, 300) in one 160 x 96 image."""
    rng = np.random.default_rng(21)
    nq, nt = 203, 300
    q, t = _desc_sets(rng, nq, nt)
    kp = np.zeros((nt, 5), np.float32)
    kp[:, 0] = rng.uniform(0, W - 0.01, nt)
    kp[:, 1] = rng.uniform(0, H - 0.01, nt)
    kp[200:290, :2] = _pile(rng, 90)   # one cell holds 90: several strides of a 16-lane row
    quv = np.stack([rng.uniform(0, W, nq), rng.uniform(0, H, nq)], 1).astype(np.float32)
    qr = np.full(nq, radius, np.float32)
    # queries 10..129 sit near a keypoint (within 0.4 px) and carry its descriptor, 12 bits flipped
    src = rng.permutation(nt)[:120]
    quv[10:130] = kp[src, :2] + rng.uniform(-0.4, 0.4, (120, 2)).astype(np.float32)
    q[10:130] = _flip(rng, t[src], 12)
    # the image corners: windows clipped on every side
    quv[130:134] = [(0, 0), (W - 0.5, 0), (0, H - 0.5), (W - 0.5, H - 0.5)]
    kp[0, :2], kp[1, :2] = (0.0, 0.0), (W - 0.25, H - 0.25)
    # the window edge: keypoint 2 + 2e exactly at u + r (kept), 3 + 2e one float above (dropped);
    # the query carries the dropped keypoint's descriptor, so a wrong edge shows as distance 0
    for e, re in enumerate(EDGE_R):
        u, v = np.float32(60.0), np.float32(10.0 + 25.0 * e)
        on = np.float32(u + np.float32(re))
        kp[2 + 2 * e, :2] = (on, v)
        kp[3 + 2 * e, :2] = (np.nextafter(on, np.float32(1e9)), v)
        quv[134 + e], qr[134 + e] = (u, v), re
        q[134 + e] = t[3 + 2 * e]
        # the same in y, on the low side
        kp[8 + 2 * e, :2] = (100.0, np.float32(v - np.float32(re)))
        kp[9 + 2 * e, :2] = (100.0, np.nextafter(np.float32(v - np.float32(re)), np.float32(-1e9)))
        quv[137 + e], qr[137 + e] = (100.0, v), re
        q[137 + e] = t[9 + 2 * e]
    quv[140] = (np.nan, 40.0)
    quv[141] = (30.0, np.inf)
    qr[142] = 0.0
    qr[143] = -2.0
    quv[144], qr[144] = (40.0, 40.0), 6.5     # the 90-keypoint cell, whatever the case's radius
    invalid = np.array([140, 141, 142, 143])
    B, q_cap, t_cap = 3, 203, 300
    Q = np.zeros((B, q_cap, 32), np.uint8)
    T = np.zeros((B, t_cap, 32), np.uint8)
    KP = np.zeros((B, t_cap, 5), np.float32)
    UV = np.zeros((B, q_cap, 2), np.float32)
    R = np.full((B, q_cap), radius, np.float32)
    Q[:], T[2], KP[2], UV[2], R[2] = q, t, kp, quv, qr     # the same queries for every item
    T[1, 0], KP[1, 0, :2], UV[1, 0] = t[7], (20.0, 20.0), (21.0, 19.0)
    T[0], KP[0] = t, kp                                    # rows beyond nt = 0 must not be read
    UV[0], UV[1, 1:] = quv, quv[1:]
    return Q, UV, R, np.array([0, 1, nq], np.int32), T, KP, np.array([0, 1, nt], np.int32), invalid


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("radius", RADII)
def test_window_knn2(radius, shared):
    from slam355 import matcher

    Q, UV, R, nq, T, KP, nt, invalid = _search_scene(radius)
    B = 3
    dq = _dev(Q[0] if shared else Q)
    duv, dr, dnq, dt, dkp, dnt = map(_dev, (UV, R, nq, T, KP, nt))
    for cell in (16, 32):
        grid = matcher.KeypointGrid(dkp, dnt, W, H, cell)
        for max_dist, ratio in SETTINGS:
            i2, d2, g = matcher.window_knn2_batch(dq, duv, dr, dnq, dt, dkp, dnt, grid,
                                                  max_dist=max_dist, ratio=ratio)
            i2, d2, g = i2.cpu().numpy(), d2.cpu().numpy(), g.cpu().numpy()
            for b in range(B):
                n = nq[b]
                ei2, ed2, eg = gr.window_knn2(Q[b, :n], UV[b, :n], R[b, :n], T[b], KP[b], nt[b],
                                              W, H, max_dist, ratio)
                assert np.array_equal(i2[b, :n], ei2), (cell, max_dist, b)
                assert np.array_equal(d2[b, :n], ed2), (cell, max_dist, b)
                assert np.array_equal(g[b, :n], eg), (cell, max_dist, b)
                # rows >= nq are not written
                assert (i2[b, n:] == -1).all() and (d2[b, n:] == -1).all() and not g[b, n:].any()
    # what the scene is there to show (last setting: max_dist 0, ratio 1/1; cell 32)
    ei2, ed2, eg = gr.window_knn2(Q[2], UV[2], R[2], T[2], KP[2], nt[2], W, H, 256, (7, 10))
    assert (ei2[invalid] == -1).all() and not eg[invalid].any()
    for e in range(len(EDGE_R)):
        for qi, kept, dropped in ((134 + e, 2 + 2 * e, 3 + 2 * e), (137 + e, 8 + 2 * e, 9 + 2 * e)):
            cand = gr.candidates(UV[2, qi, 0], UV[2, qi, 1], R[2, qi], KP[2], nt[2], W, H)
            assert kept in cand and dropped not in cand, (qi, cand)
            assert ed2[qi, 0] > 0          # the query carries the dropped keypoint's descriptor
    assert ei2[144, 1] >= 0
    if radius <= 7.0:
        assert (ei2[:, 0] == -1).sum() > len(invalid)                  # empty windows
        assert ((ei2[:, 0] >= 0) & (ei2[:, 1] == -1)).any()            # exactly one candidate
    if radius == 200.0:
        ok = np.setdiff1d(np.arange(203), np.r_[invalid, 134:140, 144])  # their own radii
        oi2, od2, _ = oracle.hamming_knn2(Q[2], T[2])
        i2, d2, _ = matcher.window_knn2_batch(dq, duv, dr, dnq, dt, dkp, dnt, grid, max_dist=256)
        assert np.array_equal(i2[2].cpu().numpy()[ok], oi2[ok])
        assert np.array_equal(d2[2].cpu().numpy()[ok], od2[ok])
        assert (od2[:10] == 0).all()                                   # ties among duplicates


@pytest.mark.gpu
def test_unique_matches():
    from slam355 import matcher

    rng = np.random.default_rng(31)
    # item 0: hand-made.  kp0 <- L0, L1 (same descriptor, same uv): L0 keeps it;
    # kp1 <- L2 (3 bits off), L3 (1 bit off): L3 keeps it; kp2 <- L4 alone.
    t = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    kp0 = np.zeros((3, 5), np.float32)
    kp0[:, :2] = [(20, 20), (80, 50), (140, 80)]
    q0 = np.stack([t[0], t[0], _flip(rng, t[1], 3), _flip(rng, t[1], 1), t[2]])
    uv0 = np.array([(21, 20), (21, 20), (80, 51), (79, 50), (140, 80)], np.float32)
    # item 1: the crowded search scene at radius 20, where many queries want the same keypoint
    Q, UV, R, nq, T, KP, nt, _ = _search_scene(20.0)
    B, q_cap, t_cap = 2, 203, 300
    q = np.zeros((B, q_cap, 32), np.uint8)
    uv = np.zeros((B, q_cap, 2), np.float32)
    tt = np.zeros((B, t_cap, 32), np.uint8)
    kp = np.zeros((B, t_cap, 5), np.float32)
    q[0, :5], uv[0, :5], tt[0, :3], kp[0, :3] = q0, uv0, t, kp0
    q[1], uv[1], tt[1], kp[1] = Q[2], UV[2], T[2], KP[2]
    r = np.full((B, q_cap), 20.0, np.float32)
    r[1] = R[2]
    n_q, n_t = np.array([5, 203], np.int32), np.array([3, 300], np.int32)
    dq, duv, dr, dnq, dt, dkp, dnt = map(_dev, (q, uv, r, n_q, tt, kp, n_t))
    grid = matcher.KeypointGrid(dkp, dnt, W, H, 32)
    i2, d2, g = matcher.window_knn2_batch(dq, duv, dr, dnq, dt, dkp, dnt, grid, max_dist=256,
                                          ratio=(1, 1))
    owner, good = matcher.unique_matches(i2, d2, g, dnq, t_cap)
    rows, count = matcher.track_rows(i2, good, dnq, dkp, 7)
    i2, d2, g = i2.cpu().numpy(), d2.cpu().numpy(), g.cpu().numpy()
    owner, good = owner.cpu().numpy(), good.cpu().numpy()
    rows, count = rows.cpu().numpy(), count.cpu().numpy()
    for b in range(B):
        n = n_q[b]
        eo, eg = gr.unique(i2[b, :n], d2[b, :n], g[b, :n], t_cap)
        assert np.array_equal(owner[b], eo) and np.array_equal(good[b, :n], eg), b
        er = gr.track_rows(i2[b, :n], eg, kp[b], 7 + b)
        assert count[b] == len(er) and np.array_equal(rows[b, :count[b]], er), b
    assert g[0, :5].all()                                   # all five wanted a keypoint
    assert list(owner[0, :3]) == [0, 3, 4] and list(good[0, :5]) == [1, 0, 0, 1, 1]
    assert g[1].sum() > good[1].sum() > 0                   # the crowded item had losers
    assert np.array_equal(np.sort(owner[1][owner[1] >= 0]), np.nonzero(good[1])[0])


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [True, False])
def test_project_landmarks(shared):
    from scipy.spatial.transform import Rotation
    from slam355 import geometry

    rng = np.random.default_rng(41)
    Wp, Hp, margin, min_depth = 640, 480, 3.0, 0.1
    P = np.array([[500.0, 0, 320.0, 0], [0, 500.0, 240.0, 0], [0, 0, 1.0, 0]])
    poses = np.tile(np.eye(4), (4, 1, 1))              # pose 0: identity (exact depths)
    for b in range(1, 4):
        poses[b, :3, :3] = Rotation.from_rotvec(rng.normal(0, 0.05, 3)).as_matrix()
        poses[b, :3, 3] = rng.normal(0, 0.3, 3)
    # in front and inside, outside each border, behind the camera, at min_depth
    z = rng.uniform(2, 30, 4000)
    X = np.stack([rng.uniform(-0.9, 0.9, 4000) * z, rng.uniform(-0.7, 0.7, 4000) * z, z], 1)
    X[:200, 2] *= -1.0
    X[200:210, 2] = min_depth                          # xc2 == min_depth under pose 0: not valid
    X[210:220, 2] = np.nextafter(min_depth, 1.0)
    X[200:220, :2] = rng.uniform(-0.03, 0.03, (20, 2))
    # no u, v within 1e-3 px of a boundary, no depth within 1e-9 of min_depth (but pose 0's exact ones)
    keep = np.ones(len(X), bool)
    for b in range(4):
        T = poses[b]
        xc = (X - T[:3, 3]) @ T[:3, :3]
        with np.errstate(all="ignore"):
            u, v = 500 * xc[:, 0] / xc[:, 2] + 320, 500 * xc[:, 1] / xc[:, 2] + 240
        for val, lim in ((u, Wp), (v, Hp)):
            keep &= ~(np.abs(val - margin) < 1e-3) & ~(np.abs(val - (lim - margin)) < 1e-3)
        if b:
            keep &= np.abs(xc[:, 2] - min_depth) > 1e-9
    keep[220:] &= np.abs(X[220:, 2]) > 0.5
    X = X[keep][:500]
    assert len(X) == 500
    n = np.array([500, 499, 0, 250], np.int32)
    Xd = _dev(X if shared else np.tile(X, (4, 1, 1)))
    uv, zc = geometry.project_landmarks(Xd, _dev(n), _dev(poses), P, Wp, Hp, margin=margin,
                                        min_depth=min_depth)
    uv, zc = uv.cpu().numpy(), zc.cpu().numpy()
    exact = total = 0
    for b in range(4):
        euv, ez = gr.project(X[:n[b]], poses[b], P, Wp, Hp, margin, min_depth)
        got = uv[b, :n[b]]
        assert np.array_equal(np.isnan(got), np.isnan(euv)), b
        assert np.isnan(uv[b, n[b]:]).all()            # rows >= nx untouched
        ok = ~np.isnan(euv[:, 0])
        ulp = np.abs(got[ok].view(np.int32).astype(np.int64) - euv[ok].view(np.int32))
        assert ulp.max(initial=0) <= 1, (b, ulp.max())
        assert np.allclose(zc[b, :n[b]], ez, rtol=1e-14, atol=0)
        exact += int((ulp == 0).sum())
        total += ulp.size
    print(f"project_landmarks: {exact} of {total} uv components bit-equal to the reference")
    euv, ez = gr.project(X, poses[0], P, Wp, Hp, margin, min_depth)
    v0 = ~np.isnan(euv[:, 0])
    assert 100 < v0.sum() < 400                        # a real mixture
    at = np.nonzero(X[:, 2] == min_depth)[0]
    assert len(at) and not v0[at].any() and v0[np.nonzero(X[:, 2] == np.nextafter(min_depth, 1.0))[0]].all()
    assert (ez < 0).any() and (euv[v0] >= margin).all()


def _yaw_pose(x, yaw):
    T = np.eye(4)
    c, s = np.cos(yaw), np.sin(yaw)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[0, 3] = x
    return T


def _e2e_scene():
    """300 landmarks seen from four frames; the poses handed to observe are off
    by 0.1 in x and 0.004 rad in yaw (predictions 10-11 px off)."""
    rng = np.random.default_rng(2024)
    Wp, Hp, nl, nf, cap = 640, 480, 300, 4, 448
    P = np.array([[500.0, 0, 320.0, 0], [0, 500.0, 240.0, 0], [0, 0, 1.0, 0]])
    X = np.stack([rng.uniform(-6, 6, nl), rng.uniform(-4, 4, nl), rng.uniform(6, 20, nl)], 1)
    D = rng.integers(0, 256, (nl, 32), dtype=np.uint8)
    true = [_yaw_pose(0.4 * f, 0.02 * f) for f in range(nf)]
    pred = np.stack([_yaw_pose(0.4 * f + 0.1, 0.02 * f + 0.004) for f in range(nf)])
    kp = np.zeros((nf, cap, 5), np.float32)
    desc = np.zeros((nf, cap, 32), np.uint8)
    n_kp = np.zeros(nf, np.int32)
    truth = np.full((nf, cap), -1, np.int64)            # keypoint -> landmark
    both = np.zeros((nf, nl), bool)                     # in view under the true and the predicted pose
    for f in range(nf):
        uv, _ = gr.project(X, true[f], P, Wp, Hp, 2.0, 0.1)   # noise of 1.5 px stays inside
        vis = np.nonzero(~np.isnan(uv[:, 0]))[0]
        both[f] = ~np.isnan(uv[:, 0]) & ~np.isnan(gr.project(X, pred[f], P, Wp, Hp)[0][:, 0])
        pts = uv[vis].astype(np.float64) + rng.uniform(-1.5, 1.5, (len(vis), 2))
        des = _flip(rng, D[vis], 20)
        pts = np.r_[pts, np.stack([rng.uniform(0, Wp, 100), rng.uniform(0, Hp, 100)], 1)]
        des = np.r_[des, rng.integers(0, 256, (100, 32), dtype=np.uint8)]
        lm = np.r_[vis, np.full(100, -1)]
        order = rng.permutation(len(pts))
        m = len(pts)
        kp[f, :m, :2], desc[f, :m], truth[f, :m], n_kp[f] = pts[order], des[order], lm[order], m
    return dict(W=Wp, H=Hp, P=P, X=X, D=D, pred=pred, kp=kp, desc=desc, n_kp=n_kp, truth=truth,
                both=both, cap=cap, nl=nl, nf=nf)


def _observe(s, lm=None):
    from slam355.mapping import LandmarkMap

    if lm is None:
        lm = LandmarkMap(s["nl"], s["cap"], s["W"], s["H"], s["P"]).add(s["X"], s["D"])
    args = (_dev(s["pred"]), _dev(s["kp"]), _dev(s["desc"]), _dev(s["n_kp"]))
    return lm, args


@pytest.mark.gpu
def test_landmark_map_end_to_end():
    from slam355 import XXXport_files as xf

    s = _e2e_scene()
    lm, args = _observe(s)
    rows, count = lm.observe(0, *args, radius=15.0, max_dist=64, ratio=(7, 10))
    rows, count = rows.cpu().numpy(), count.cpu().numpy()
    uv = lm.uv.cpu().numpy()
    seen = np.zeros((s["nf"], s["nl"]), bool)
    for f in range(s["nf"]):
        # the reference on the GPU's own uv (the projection has its own test)
        qr = np.full(s["nl"], 15.0, np.float32)
        i2, d2, g = gr.window_knn2(s["D"], uv[f], qr, s["desc"][f], s["kp"][f], s["n_kp"][f],
                                   s["W"], s["H"], 64, (7, 10))
        owner, good = gr.unique(i2, d2, g, s["cap"])
        er = gr.track_rows(i2, good, s["kp"][f], f)
        assert count[f] == len(er) and np.array_equal(rows[f, :count[f]], er), f
        assert np.array_equal(lm.idx2[f].cpu().numpy(), i2)
        assert np.array_equal(lm.dist2[f].cpu().numpy(), d2)
        assert np.array_equal(lm.good[f].cpu().numpy(), good)
        assert np.array_equal(lm.owner[f].cpu().numpy(), owner)
        # every row's keypoint is the landmark's true one, and nothing in view was missed
        r = rows[f, :count[f]]
        l = r[:, 1].astype(int)
        j = i2[l, 0]
        assert np.array_equal(s["truth"][f, j], l), f
        assert np.array_equal(s["kp"][f, j, :2].astype(np.float64), r[:, 2:]), f
        seen[f, l] = True
        assert seen[f][s["both"][f]].all(), f
        print(f"frame {f}: {count[f]} of {s['nl']} landmarks matched, {s['both'][f].sum()} in view "
              "under both poses")
    full = int(seen.all(0).sum())
    print(f"{full} tracks of length {s['nf']}")
    assert full >= 250
    om, ids = lm.tracks(compact=True)
    assert len(om) == count.sum() and np.array_equal(ids, np.nonzero(seen.any(0))[0])
    frames = [s["pred"][f] for f in range(s["nf"])] + [s["pred"][-1]]   # + the trailing frame
    cams, pts, ci, pi, qs = xf.problem_from_map(om, frames, s["X"][ids], s["P"])
    assert cams.shape == (s["nf"], 9) and len(pts) == len(ids) and len(qs) == len(om)
    assert (np.bincount(pi, minlength=len(pts)) >= 1).all()
    assert np.array_equal(lm.tracks()[:, 1], ids[om[:, 1].astype(int)])


@pytest.mark.gpu
def test_observe_in_graph_capture():
    import torch

    s = _e2e_scene()
    lm, args = _observe(s)
    want, want_n = lm.observe(0, *args)          # eager; also allocates the per-batch buffers
    want, want_n = want.cpu().numpy(), want_n.cpu().numpy()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rows, count = lm.observe(0, *args)       # a host sync or a hipMalloc here fails the capture
    rows.zero_()
    count.zero_()
    g.replay()
    torch.cuda.synchronize()
    count = count.cpu().numpy()
    assert np.array_equal(count, want_n) and count.min() > 200
    for f in range(s["nf"]):
        assert np.array_equal(rows[f, :count[f]].cpu().numpy(), want[f, :want_n[f]])
