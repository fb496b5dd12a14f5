"""Plain NumPy restatement of relocalization (include/slam355.h,
"Relocalization"): the Hamming kNN-2 against the live map, the rows and PnP
inputs from the owners, the start pose from PnP's result, and the whole chain
of LandmarkMap.relocalize for one frame (uniqueness from guided_ref, PnP from
the CPU oracle, refinement from pose_refine_ref).  Also the revisit scene the
CPU and the GPU tests share.  Test infrastructure only; every function works on
ONE batch item."""
import functools

import numpy as np

import guided_ref as gr
import pose_refine_ref as pr

_POP = np.array([bin(i).count("1") for i in range(256)], np.uint8)
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def _popcount64(a):
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(a)
    return _POP[a.view(np.uint8).reshape(a.shape + (8,))].sum(-1, dtype=np.uint8)


def eligible(X, last, n, lo, hi):
    """Indices of the landmarks below the clamped count that are alive and have lo <= last < hi."""
    n = min(max(int(n), 0), len(X))
    ok = ~np.isnan(X[:n, 0]) & (last[:n] >= lo) & (last[:n] < hi)
    return np.nonzero(ok)[0]


def map_knn2(q, nq, desc, X, last, n, lo, hi, max_dist=64, ratio=(7, 10)):
    """q [q_cap,32] u8 -> (idx2, dist2 [q_cap,2] i32, good [q_cap] u8); rows >= nq
    stay -1 / -1 / 0.  Sequential over chunks of queries, no large temporaries."""
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
    q_cap = len(q)
    nq = min(max(int(nq), 0), q_cap)
    idx2 = np.full((q_cap, 2), -1, np.int32)
    dist2 = np.full((q_cap, 2), -1, np.int32)
    good = np.zeros(q_cap, np.uint8)
    el = eligible(X, last, n, lo, hi)
    if len(el) == 0:
        return idx2, dist2, good
    t64 = np.ascontiguousarray(desc[el]).view(np.uint64)            # [E, 4]
    q64 = q.view(np.uint64)
    num, den = ratio
    for c0 in range(0, nq, 16):
        c1 = min(c0 + 16, nq)
        D = _popcount64(q64[c0:c1, None, :] ^ t64[None, :, :]).sum(2, dtype=np.int64)  # [c, E]
        key = (D << 20) | el[None, :]
        for i in range(c0, c1):
            k = np.sort(key[i - c0])[:2]
            for s, v in enumerate(k):
                idx2[i, s], dist2[i, s] = v & 0xFFFFF, v >> 20
            if len(k) == 2:
                d1, d2 = int(dist2[i, 0]), int(dist2[i, 1])
                good[i] = d1 <= max_dist and den * d1 < num * d2
    return idx2, dist2, good


def reloc_rows(owner, n, kp, X, frame):
    """owner [x_cap] i32 (the keypoint a landmark won, or -1) -> (rows [k,4], Q [k,3], q [k,2])."""
    kp = np.asarray(kp, np.float32)
    n = min(max(int(n), 0), len(owner))
    i = np.nonzero((owner[:n] >= 0) & (owner[:n] < len(kp)))[0]
    j = owner[i]
    xy = kp[j, :2].astype(np.float64).reshape(-1, 2)
    rows = np.concatenate([np.full((len(i), 1), float(frame)), i[:, None].astype(np.float64), xy], 1)
    return rows, X[i].reshape(-1, 3).copy(), xy.copy()


def reloc_pose(rvec, tvec, ninl, count, P, prior, min_inliers):
    """-> (camera-to-world pose 4x4, count_out)."""
    if ninl < min_inliers:
        return (np.eye(4) if prior is None else np.array(prior, np.float64).reshape(4, 4)), 0
    P = np.asarray(P, np.float64).reshape(3, 4)
    s2 = P[2, 3] / P[2, 2]
    s1 = (P[1, 3] - P[1, 2] * s2) / P[1, 1]
    s0 = ((P[0, 3] - P[0, 1] * s1) - P[0, 2] * s2) / P[0, 0]
    T = np.eye(4)
    T[:3, :3] = pr.rodrigues(np.asarray(rvec, np.float64)).T
    T[:3, 3] = -T[:3, :3] @ (np.asarray(tvec, np.float64) - [s0, s1, s2])
    return T, int(count)


REFINE = dict(loss=1, loss_scale=2.4477, gate=2.4477, min_depth=0.1, n_rounds=4, iters=10)


def relocalize(m, kp, desc, n_kp, P, frame, lo=INT_MIN, hi=INT_MAX, prior=None, max_dist=64,
               ratio=(7, 10), seed=0, item=0, min_inliers=10, start=None):
    """LandmarkMap.relocalize for one frame on a map dict of map_life_ref ->
    dict(rows, owner, Q, q, pnp=(rvec, tvec, ninl, mask), start, count, refined).
    start: refine from this pose instead of the chain's own (the GPU's start pose)."""
    from oracle import geometry as og

    cap = len(m["X"])
    i2, d2, g = map_knn2(desc, n_kp, m["desc"], m["X"], m["last"], m["n"], lo, hi, max_dist, ratio)
    owner, _ = gr.unique(i2, d2, g, cap)
    assert not np.isnan(m["X"][owner >= 0, 0]).any()     # uniqueness only sees eligible landmarks
    assert (owner[m["n"]:] == -1).all()
    rows, Q, q = reloc_rows(owner, m["n"], kp, m["X"], frame)
    K = np.asarray(P, np.float64).reshape(3, 4)[:, :3]
    rvec, tvec, ninl, mask = og.pnp_ransac(Q, q, K, seed=seed, item=item)
    pose0, count = reloc_pose(rvec, tvec, ninl, len(rows), P, prior, min_inliers)
    begin = pose0 if start is None else np.asarray(start, np.float64).reshape(4, 4)
    refined = pr.refine(rows, count, m["X"], begin, P, min_inliers=min_inliers, **REFINE)
    return dict(rows=rows, owner=owner, Q=Q, q=q, pnp=(rvec, tvec, ninl, mask), start=pose0,
                count=count, refined=refined)


# ----------------------------------------------------------------------------- the revisit scene
@functools.lru_cache(maxsize=None)
def revisit_scene():
    """The final map of test_map_life's reference life cycle, revisited: three
    frames from new viewpoints.  A frame's keypoints are the live landmarks in
    view (+-1 px, 20 flipped descriptor bits), 40 clutter keypoints with random
    descriptors and 30 impostors -- the descriptor (5 flipped bits) of a live
    landmark NOT in view, at a random pixel.  The prior is 2.5 m and 0.12 rad
    off; frame 3 is clutter only."""
    import test_map_life as tml

    m = tml._reference_run(True)["map"]
    rng = np.random.default_rng(77)
    W, H, P3, cap = tml.W, tml.H, tml.P3, 512             # cap: keypoints per frame
    views = [(4.0, 0.05), (11.3, -0.04), (17.6, 0.11)]
    poses = views + [(9.0, 0.0)]
    nf = len(poses)
    true = np.stack([tml._yaw_pose(x, yaw) for x, yaw in poses])
    prior = np.stack([tml._yaw_pose(x + 2.5, yaw + 0.12) for x, yaw in poses])
    for T in (true, prior):
        T[:, 1, 3], T[:, 2, 3] = 0.2, -0.5
    n = m["n"]
    alive = ~np.isnan(m["X"][:n, 0])
    kp = np.zeros((nf, cap, 5), np.float32)
    desc = np.zeros((nf, cap, 32), np.uint8)
    n_kp = np.zeros(nf, np.int32)
    kind = np.full((nf, cap), -1, np.int64)             # 0 landmark in view, 1 clutter, 2 impostor
    for f in range(nf):
        X = np.where(alive[:, None], m["X"][:n], 0.0)
        uv, _ = gr.project(X, true[f], P3, W, H, 2.0, 0.1)
        vis = np.nonzero(~np.isnan(uv[:, 0]) & alive)[0] if f < len(views) else np.zeros(0, np.int64)
        hidden = np.nonzero(np.isnan(uv[:, 0]) & alive)[0]
        imp = rng.choice(hidden, 30, replace=False) if f < len(views) else np.zeros(0, np.int64)
        ncl = 40 if f < len(views) else 300
        pts = np.r_[uv[vis].astype(np.float64) + rng.uniform(-1.0, 1.0, (len(vis), 2)),
                    np.stack([rng.uniform(0, W, ncl + len(imp)), rng.uniform(0, H, ncl + len(imp))], 1)]
        des = np.r_[tml._flip(rng, m["desc"][vis], 20),
                    rng.integers(0, 256, (ncl, 32), dtype=np.uint8),
                    tml._flip(rng, m["desc"][imp], 5).reshape(-1, 32)]
        kd = np.r_[np.zeros(len(vis), np.int64), np.ones(ncl, np.int64), np.full(len(imp), 2)]
        order = rng.permutation(len(pts))
        k = len(pts)
        assert k <= cap
        kp[f, :k, :2], desc[f, :k], kind[f, :k], n_kp[f] = pts[order], des[order], kd[order], k
    return dict(map=m, true=true, prior=prior, kp=kp, desc=desc, n_kp=n_kp, kind=kind, cap=cap,
                x_cap=len(m["X"]), W=W, H=H, P=P3, nf=nf, nviews=len(views))
