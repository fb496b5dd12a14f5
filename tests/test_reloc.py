"""Relocalization on the GPU: slam_hamming_map_knn2, slam_reloc_rows and
slam_reloc_pose against tests/reloc_ref.py, LandmarkMap.relocalize on the
revisit scene, in a captured graph, and as the source of a pose-graph edge.

Bars: the matcher and the rows are integer or copied data and must be
bit-exact; slam_reloc_pose agrees with NumPy to 1e-12; the PnP stage meets
test_gpu_pnp_matches_oracle's bars (count, mask, 1e-8) and the refinement those
of tests/test_pose_refine.py, the reference fed the GPU's own start pose."""
import numpy as np
import pytest

import pose_refine_ref as pr
import reloc_ref as rr

pytestmark = pytest.mark.gpu
ALL = (rr.INT_MIN, rr.INT_MAX)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _segment():
    from slam355 import matcher

    return matcher.MAP_KNN_SEGMENT


# ----------------------------------------------------------------------------- slam_hamming_map_knn2
def _knn_gpu(q, nq, desc, X, last, n, ranges, max_dist=64, ratio=(7, 10)):
    import torch
    from slam355 import matcher

    B, q_cap = q.shape[:2]
    out = (torch.full((B, q_cap, 2), -7, dtype=torch.int32, device="cuda"),
           torch.full((B, q_cap, 2), -7, dtype=torch.int32, device="cuda"),
           torch.full((B, q_cap), 9, dtype=torch.uint8, device="cuda"))
    ins = [_dev(q), _dev(np.asarray(nq, np.int32)), _dev(desc), _dev(X), _dev(last),
           _dev(np.array([n], np.int32)), _dev(np.asarray(ranges, np.int32))]
    matcher.map_knn2_batch(*ins, max_dist=max_dist, ratio=ratio, out=out)
    return [t.cpu().numpy() for t in out]


def _knn_check(q, nq, desc, X, last, n, ranges, max_dist=64, ratio=(7, 10)):
    """GPU against the reference, bit for bit -> the reference's (idx2, dist2, good) per item."""
    got = _knn_gpu(q, nq, desc, X, last, n, ranges, max_dist, ratio)
    wants = []
    for b in range(len(q)):
        want = rr.map_knn2(q[b], nq[b], desc, X, last, n, ranges[b][0], ranges[b][1], max_dist, ratio)
        k = min(max(int(nq[b]), 0), q.shape[1])
        for g, w, untouched in zip(got, want, (-7, -7, 9)):
            assert np.array_equal(g[b, :k], w[:k]), (b, k)
            assert (g[b, k:] == untouched).all(), b          # rows >= nq are not written
        wants.append(want)
    return wants


def _map(rng, count, x_cap, q_cap):
    """A random map of `count` landmarks (a fifth dead) in x_cap slots, and q_cap
    queries 3 bits off landmark t[j]; the slots past `count` hold exact copies of
    the queries, alive and in every range: they would win if they were read."""
    desc = rng.integers(0, 256, (x_cap, 32), dtype=np.uint8)
    X = rng.normal(0, 5, (x_cap, 3))
    last = rng.integers(0, 20, x_cap).astype(np.int32)
    dead = rng.random(x_cap) < 0.2
    X[dead, 0] = np.nan
    X[dead & (rng.random(x_cap) < 0.5), 1:] = np.nan
    t = rng.integers(0, max(count, 1), q_cap)
    q = desc[t].copy()
    q[:, 0] ^= 0x07
    k = x_cap - count
    desc[count:] = q[np.arange(k) % q_cap]
    X[count:], last[count:] = 1.0, 6
    return desc, X, last, q, t


NQ = [0, 1, 63, 64, 65, 129, -3]
RANGES = [ALL, (5, 12), (0, 3)]


@pytest.mark.parametrize("segs,more", [(0, 0), (0, 1), (0, 2), (1, -1), (1, 0), (1, 1), (3, 5)])
def test_map_knn2_landmark_and_query_counts(segs, more):
    count = segs * _segment() + more
    rng = np.random.default_rng(count)
    q_cap, x_cap = 130, count + 9
    desc, X, last, q, t = _map(rng, count, x_cap, q_cap)
    B = len(NQ)
    ranges = [RANGES[b % 3] for b in range(B)]
    if count >= 64:      # last exactly lo: eligible; exactly hi: not (item 4 has the range (5, 12))
        t[1] = (t[0] + 1) % count
        q[:2] = desc[t[:2]]
        q[:2, 0] ^= 0x07
        X[t[:2]] = 1.0
        last[t[0]], last[t[1]] = 5, 12
    qs = np.stack([q] * B)
    want = _knn_check(qs, NQ, desc, X, last, count, ranges)
    if count >= 64:
        i2, d2, _ = want[4]
        assert i2[0, 0] == t[0] and d2[0, 0] == 3 and i2[1, 0] != t[1]
        dead_best = np.isnan(X[t[:64], 0])                  # dead landmarks that would be nearest (item 3: every range)
        assert dead_best.any() and (want[3][0][:64][dead_best, 0] != t[:64][dead_best]).all()
        assert (want[3][0][:64][~dead_best, 0] == t[:64][~dead_best]).all()
    assert all((w[0] < count).all() for w in want)          # nothing from the stale slots


def test_map_knn2_beyond_16_bits_and_ties_across_segments():
    S = _segment()
    rng = np.random.default_rng(70000)
    count, x_cap, q_cap = 70000, 70016, 129
    desc, X, last, q, t = _map(rng, count, x_cap, q_cap)
    t[:40] = 65536 + 7 * np.arange(40)                      # true neighbours past 16 bits
    q[:40] = desc[t[:40]]
    q[:40, 0] ^= 0x07
    lo_i, hi_i = 100, 69000                                 # equal descriptors in two segments
    assert lo_i // S != hi_i // S
    desc[lo_i] = desc[hi_i] = q[50]
    for i in list(t[:40]) + [lo_i, hi_i]:
        X[i], last[i] = 1.0, 6
    qs = np.stack([q, q])
    want = _knn_check(qs, [129, 64], desc, X, last, count, [ALL, (5, 12)])
    for i2, d2, good in want:
        assert (i2[:40, 0] == t[:40]).all() and (d2[:40, 0] == 3).all()
        assert i2[50].tolist() == [lo_i, hi_i] and d2[50].tolist() == [0, 0] and good[50] == 0


def test_map_knn2_one_and_no_eligible_landmark():
    S = _segment()
    rng = np.random.default_rng(3)
    count = S + 1
    desc, X, last, q, _ = _map(rng, count, count + 4, 65)
    X[S], last[S] = 1.0, 1000                               # alone in the second segment and in its range
    want = _knn_check(np.stack([q, q]), [65, 65], desc, X, last, count, [(1000, 1001), (2000, 2001)])
    assert (want[0][0][:, 0] == S).all() and (want[0][0][:, 1] == -1).all() and not want[0][2].any()
    assert (want[1][0] == -1).all() and (want[1][1] == -1).all() and not want[1][2].any()


@pytest.mark.parametrize("max_dist,ratio", [(0, (7, 10)), (256, (1, 1))])
def test_map_knn2_max_dist_and_ratio(max_dist, ratio):
    rng = np.random.default_rng(max_dist)
    count = 300
    desc, X, last, q, t = _map(rng, count, count, 64)
    q[:10] = desc[t[:10]]                                   # exact copies: d1 = 0
    X[t[:10]] = 1.0
    want = _knn_check(q[None], [64], desc, X, last, count, [ALL], max_dist, ratio)
    good = want[0][2]
    if max_dist == 0:
        assert good[:10].all() and not good[10:][want[0][1][10:, 0] > 0].any()
    else:
        assert good.sum() > 10


# ----------------------------------------------------------------------------- slam_reloc_rows / slam_reloc_pose
@pytest.mark.parametrize("x_cap", [1, 255, 256, 257, 1025])
def test_reloc_rows_against_reference(x_cap):
    import torch
    from slam355 import _lib
    from slam355.device import ptr

    rng = np.random.default_rng(x_cap)
    B, kp_cap = 3, x_cap + 3
    rows_cap = x_cap
    n = x_cap if x_cap < 3 else x_cap - 2
    owner = np.full((B, x_cap), -1, np.int32)
    owner[1] = rng.permutation(kp_cap)[:x_cap]              # all taken
    owner[2, ::2] = rng.permutation(kp_cap)[:len(owner[2, ::2])]   # alternating
    owner[0, n:] = 1                                        # stale entries past the count
    kp = rng.uniform(0, 600, (B, kp_cap, 5)).astype(np.float32)
    X = rng.normal(0, 5, (x_cap, 3))
    d_rows = torch.full((B, rows_cap, 4), -3.0, dtype=torch.float64, device="cuda")
    d_Q = torch.full((B, rows_cap, 3), -3.0, dtype=torch.float64, device="cuda")
    d_q = torch.full((B, rows_cap, 2), -3.0, dtype=torch.float64, device="cuda")
    d_cnt = torch.full((B,), -3, dtype=torch.int32, device="cuda")
    ins = [_dev(owner), _dev(np.array([n], np.int32)), _dev(kp), _dev(X)]
    _lib.call("slam_reloc_rows", ptr(ins[0]), ptr(ins[1]), x_cap, ptr(ins[2]), kp_cap, ptr(ins[3]), B,
              40, rows_cap, ptr(d_rows), ptr(d_cnt), ptr(d_Q), ptr(d_q), None)
    rows, Q, q, cnt = (t.cpu().numpy() for t in (d_rows, d_Q, d_q, d_cnt))
    for b in range(B):
        wr, wQ, wq = rr.reloc_rows(owner[b], n, kp[b], X, 40 + b)
        k = len(wr)
        assert cnt[b] == k == (0, n, (n + 1) // 2)[b]
        assert np.array_equal(rows[b, :k], wr) and np.array_equal(Q[b, :k], wQ) and np.array_equal(q[b, :k], wq)
        assert (rows[b, k:] == -3.0).all() and (Q[b, k:] == -3.0).all() and (q[b, k:] == -3.0).all()


@pytest.mark.parametrize("with_prior", [True, False])
def test_reloc_pose_against_numpy(with_prior):
    import torch
    from slam355 import _lib
    from slam355.device import ptr

    rng = np.random.default_rng(12)
    B, min_inl = 5, 10
    P = np.array([[500.0, 0.3, 320.0, -270.0], [0, 480.0, 240.0, 12.0], [0, 0, 1.0, 0.004]])
    rvec, tvec = rng.normal(0, 0.7, (B, 3)), rng.normal(0, 3, (B, 3))
    rvec[3] = 0.0                                           # the identity branch of Rodrigues
    ninl = np.array([50, 3, -1, 10, 9], np.int32)
    count = np.array([80, 30, 4, 17, 12], np.int32)
    prior = rng.normal(0, 1, (B, 4, 4)) if with_prior else None
    d_pose = torch.full((B, 4, 4), 9.0, dtype=torch.float64, device="cuda")
    d_cnt = torch.full((B,), -3, dtype=torch.int32, device="cuda")
    ins = [_dev(rvec), _dev(tvec), _dev(ninl), _dev(count), _dev(P), _dev(prior) if with_prior else None]
    _lib.call("slam_reloc_pose", *(ptr(t) for t in ins), B, min_inl, ptr(d_pose), ptr(d_cnt), None)
    pose, cnt = d_pose.cpu().numpy(), d_cnt.cpu().numpy()
    for b in range(B):
        want, wc = rr.reloc_pose(rvec[b], tvec[b], ninl[b], count[b], P, None if prior is None else prior[b],
                                 min_inl)
        assert cnt[b] == wc == (count[b] if ninl[b] >= min_inl else 0)
        if ninl[b] < min_inl:
            assert np.array_equal(pose[b].view(np.uint64), want.view(np.uint64)), b     # bit for bit
            continue
        err = np.abs(pose[b] - want).max()
        print(f"frame {b}: start pose against NumPy {err:.2e}")
        assert err <= 1e-12 and np.array_equal(pose[b, 3], [0.0, 0.0, 0.0, 1.0])
        # the pose reproduces PnP's projection through the whole P
        Xw = rng.normal(0, 2, 3) + [0, 0, 8]
        h1 = P[:, :3] @ (pr.rodrigues(rvec[b]) @ Xw + tvec[b])
        h2 = P[:, :3] @ (pose[b, :3, :3].T @ (Xw - pose[b, :3, 3])) + P[:, 3]
        assert np.allclose(h1, h2, rtol=1e-10, atol=1e-10)


# ----------------------------------------------------------------------------- LandmarkMap.relocalize
def _landmark_map(s, n=None):
    from slam355.mapping import LandmarkMap

    m = s["map"]
    lm = LandmarkMap(s["x_cap"], s["cap"], s["W"], s["H"], s["P"])
    for k in ("X", "desc", "visible", "found", "born", "last"):
        getattr(lm, k).copy_(_dev(m[k]))
    lm.n = m["n"] if n is None else n
    lm.n_dev.fill_(lm.n)
    return lm


def _pose_close(a, b):
    return (np.abs(a[:3, :3] - b[:3, :3]).max() <= 1e-8 and
            np.abs(a[:3, 3] - b[:3, 3]).max() <= 1e-8 * (1.0 + np.abs(b[:3, 3]).max()))


def _check_frame(s, f, b, res, lm_state, lo=rr.INT_MIN, hi=rr.INT_MAX, m=None):
    """Frame f of the scene as item b of a relocalize call against the reference chain."""
    pose, rows, count, mask, ninl, status, info = res
    matched, pnp, start = lm_state
    m = s["map"] if m is None else m
    ref = rr.relocalize(m, s["kp"][f], s["desc"][f], s["n_kp"][f], s["P"], 100 + b, lo=lo, hi=hi,
                        prior=s["prior"][f], seed=7, item=b, start=start[b])
    k = len(ref["rows"])
    assert matched[b] == k and np.array_equal(rows[b, :k], ref["rows"]), (f, matched[b], k)
    rvec, tvec, en, emask = ref["pnp"]        # oracle.geometry.pnp_ransac on the reference's Q, q
    assert pnp[2][b] == en, (f, pnp[2][b], en)
    if en >= 0:
        assert np.array_equal(pnp[3][b, :k].astype(bool), emask), f
        assert np.allclose(pnp[0][b], rvec, rtol=0, atol=1e-8) and np.allclose(pnp[1][b], tvec, atol=1e-8), f
    want_start, want_count = rr.reloc_pose(pnp[0][b], pnp[1][b], pnp[2][b], k, s["P"], s["prior"][f], 10)
    assert count[b] == want_count == ref["count"]
    assert np.abs(start[b] - want_start).max() <= 1e-12
    two = ref["refined"]
    assert status[b] == two["status"] and ninl[b] == two["ninl"], (f, status[b], ninl[b], two["status"])
    c = count[b]
    assert np.array_equal(mask[b, :c].astype(bool), two["mask"]), f
    if two["status"] != 0:
        assert np.array_equal(pose[b].view(np.uint64), start[b].view(np.uint64)) and not info[b].any()
        return ref
    assert two["margin"] > 1e-6 and _pose_close(pose[b], two["pose"]), f
    want = pr.information_at(pose[b], mask[b, :c], ref["rows"], m["X"], s["P"], 1, 2.4477)
    assert np.abs(info[b] - want).max() <= 1e-12 * np.diag(want).max(), f
    assert np.array_equal(info[b], info[b].T)
    return ref


def _run(lm, s, frames, **kw):
    res = lm.relocalize(100, _dev(s["kp"][frames]), _dev(s["desc"][frames]), _dev(s["n_kp"][frames]),
                        prior=_dev(s["prior"][frames]), seed=7, **kw)
    res = [t.cpu().numpy().copy() for t in res]
    state = (lm.matched.cpu().numpy().copy(), [t.cpu().numpy().copy() for t in lm.pnp],
             lm.start.cpu().numpy().copy())
    return res, state


def test_relocalize_on_the_revisit_scene():
    s = rr.revisit_scene()
    lm = _landmark_map(s)
    frames = [0, 1, 2]
    res, state = _run(lm, s, frames)
    for b, f in enumerate(frames):
        ref = _check_frame(s, f, b, res, state)
        terr = np.linalg.norm(res[0][b, :3, 3] - s["true"][f, :3, 3])
        l = ref["rows"][:, 1].astype(int)
        imp = s["kind"][f][ref["owner"][l]] == 2
        print(f"frame {f}: rows {len(l)}, PnP inliers {state[1][2][b]}, refined inliers {res[4][b]}, "
              f"impostor rows {int(imp.sum())}, translation error {terr:.4f}")
        assert res[5][b] == 0 and terr < 0.03
        assert imp.any() and not res[3][b, :len(l)][imp].any()
    assert lm.tracks().shape[0] == 0 and lm.size() == s["map"]["n"]      # nothing kept, nothing changed
    # a range of `last`: the rows name only landmarks inside it
    res, state = _run(lm, s, frames, last_range=(0, 8), keep_tracks=True)
    for b, f in enumerate(frames):
        ref = _check_frame(s, f, b, res, state, lo=0, hi=8)
        l = ref["rows"][:, 1].astype(int)
        assert len(l) > 0 and (s["map"]["last"][l] < 8).all()
    assert lm.tracks().shape[0] == res[2].sum()
    # a frame of clutter only comes back with its prior, bit for bit, at status 1
    frames = [0, 3, 1]
    res, state = _run(lm, s, frames, last_range=np.array([ALL, ALL, ALL], np.int64))
    for b, f in enumerate(frames):
        _check_frame(s, f, b, res, state)
    assert res[5].tolist() == [0, 1, 0] and res[2][1] == 0 and res[4][1] == -1
    assert np.array_equal(res[0][1].view(np.uint64), s["prior"][3].view(np.uint64))


def test_relocalize_in_graph_capture():
    import torch

    s = rr.revisit_scene()
    m = s["map"]
    frames = [0, 1, 2]
    args = [_dev(s[k][frames]) for k in ("kp", "desc", "n_kp")]
    prior = _dev(s["prior"][frames])
    rng = _dev(np.array([ALL] * 3, np.int32))
    graphed = _landmark_map(s, n=600)
    graphed.relocalize(100, *args, last_range=rng, prior=prior, seed=7)    # allocates every buffer
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):    # a host sync or a hipMalloc here fails the capture
        got = graphed.relocalize(100, *args, last_range=rng, prior=prior, seed=7)
    # other ranges and a grown map, changed on the device only
    new = np.array([(0, 12), ALL, (2, 16)], np.int32)
    rng.copy_(_dev(new))
    graphed.n_dev.fill_(m["n"])
    for t in got:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in got]
    eager = _landmark_map(s)
    want = [t.cpu().numpy() for t in eager.relocalize(100, *args, last_range=_dev(new), prior=prior, seed=7)]
    count = got[2]
    assert np.array_equal(count, want[2]) and count.min() > 50
    assert (got[5] == 0).all() and np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5])
    for f in range(3):
        c = count[f]
        assert np.array_equal(got[1][f, :c], want[1][f, :c])
        assert np.array_equal(got[3][f, :c], want[3][f, :c])
        assert (m["last"][got[1][f, :c, 1].astype(int)] < new[f, 1]).all()
    assert got[1][:, :, 1].max() >= 600                     # landmarks the captured count did not cover
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[6], want[6])


# ----------------------------------------------------------------------------- the pose-graph edge
def test_relocalized_frame_closes_a_drifting_chain():
    """A chain of odometry edges from the map's origin to the revisit pose drifts;
    the edge edge_from_localization makes of the relocalized frame is consistent
    with the graph, a pose 5 m off is not, and solving with the edge pulls the
    chain's end towards the truth."""
    from slam355 import posegraph as pg

    s = rr.revisit_scene()
    lm = _landmark_map(s)
    res, _ = _run(lm, s, [0, 1, 2])
    pose, info = res[0][0], res[6][0]
    assert res[5][0] == 0

    def w2c(T):
        return np.concatenate([pg._so3_log(T[:3, :3].T), -T[:3, :3].T @ T[:3, 3]])

    def compose(x, z):
        R = pg._so3_exp(x[:3])
        return np.concatenate([pg._so3_log(R @ pg._so3_exp(z[:3])), x[3:] + R @ z[3:]])

    rng = np.random.default_rng(5)
    N, sig = 12, np.array([0.004] * 3 + [0.04] * 3)
    end = w2c(s["true"][0])
    truth = np.stack([end * k / (N - 1) for k in range(N)])
    edges = np.stack([np.arange(N - 1), np.arange(1, N)], 1)
    meas = np.stack([pg.relative_pose(truth[k], truth[k + 1]) for k in range(N - 1)])
    meas += rng.normal(0, 1, meas.shape) * sig              # the odometry's noise, at its stated information
    odo = np.tile(np.diag(1.0 / sig ** 2), (N - 1, 1, 1))
    x = [np.zeros(6)]
    for z in meas:
        x.append(compose(x[-1], z))
    x = np.stack(x)
    fixed = np.zeros(N, np.uint32)
    fixed[0] = pg.FIXED_POSE
    z_loop, W_loop = pg.edge_from_localization(x[0], pose, info)
    wrong = pose.copy()
    wrong[0, 3] += 5.0
    z_wrong, W_wrong = pg.edge_from_localization(x[0], wrong, info)
    g = pg.PoseGraph(x, edges, meas, information=odo, fixed=fixed)
    gate = g.gate([[0, N - 1], [0, N - 1]], np.stack([z_loop, z_wrong]), information=np.stack([W_loop, W_wrong]))
    before = np.linalg.norm(x[-1, 3:] - truth[-1, 3:])
    print(f"gate d2: relocalized {gate['d2'][0]:.2f}, 5 m off {gate['d2'][1]:.1f}; drift of the end {before:.3f} m")
    assert gate["accept"].tolist() == [True, False]
    g2 = pg.PoseGraph(x, np.r_[edges, [[0, N - 1]]], np.r_[meas, z_loop[None]],
                      information=np.r_[odo, W_loop[None]], fixed=fixed)
    g2.solve()
    after = np.linalg.norm(g2.poses()[-1, 3:] - truth[-1, 3:])
    print(f"after the solve {after:.4f} m")
    assert after < before
