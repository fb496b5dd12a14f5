"""Guided matching (LandmarkMap.observe's five launches) on the tracking shape:
a shared map of M landmarks against 2,087 keypoints per 1280 x 720 frame, batch
32, radius 15, cell 32 -- HIP-event time per step, of steps 2-4 and 1-5 as one
chain, and of the brute-force slam_hamming_knn2 at 2,048 x 2,087 x 32 beside it
in the same process.  One JSON line per map size.

    python scripts/guided_time.py [M ...]     (default: 2048 65536)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slam-1_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from slam355 import geometry, matcher  # noqa: E402

B, NKP, W, H, RADIUS, CELL = 32, 2087, 1280, 720, 15.0, 32
REPS, ROUNDS = 200, 5
P = np.array([[700.0, 0, 640.0, 0], [0, 700.0, 360.0, 0], [0, 0, 1.0, 0]])
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731


def scene(M, rng):
    """M landmarks in the frustum of frame 0; every frame sees up to NKP of them
    as keypoints (1 px noise, 20 flipped bits), the rest of its keypoints random."""
    z = rng.uniform(4, 40, M)
    X = np.stack([rng.uniform(-0.9, 0.9, M) * z, rng.uniform(-0.5, 0.5, M) * z, z], 1)
    D = rng.integers(0, 256, (M, 32), dtype=np.uint8)
    poses = np.tile(np.eye(4), (B, 1, 1))
    poses[:, 0, 3] = 0.05 * np.arange(B)
    kp = np.zeros((B, NKP, 5), np.float32)
    desc = rng.integers(0, 256, (B, NKP, 32), dtype=np.uint8)
    kp[..., 0] = rng.uniform(0, W, (B, NKP))
    kp[..., 1] = rng.uniform(0, H, (B, NKP))
    for b in range(B):
        xc = X - poses[b, :3, 3]
        uv = xc[:, :2] / xc[:, 2:] * 700.0 + (640.0, 360.0)
        vis = np.nonzero((uv[:, 0] >= 2) & (uv[:, 0] < W - 2) & (uv[:, 1] >= 2) & (uv[:, 1] < H - 2))[0]
        pick = rng.permutation(vis)[:min(len(vis), NKP * 3 // 4)]
        slot = rng.permutation(NKP)[:len(pick)]
        kp[b, slot, :2] = uv[pick] + rng.uniform(-1, 1, (len(pick), 2))
        bits = np.unpackbits(D[pick], axis=1)
        bits ^= (rng.random(bits.shape) < 20 / 256).astype(np.uint8)
        desc[b, slot] = np.packbits(bits, axis=1)
    poses[:, 0, 3] += 0.02      # the predicted pose is off
    return X, D, poses, kp, desc


def timed(fn):
    """Median over ROUNDS of the mean HIP-event time of REPS back-to-back calls, in us."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / REPS * 1e3)
    return float(np.median(out))


def measure(M, rng):
    X, D, poses, kp, desc = map(T, scene(M, rng))
    dev = X.device
    nq = torch.full((B,), M, dtype=torch.int32, device=dev)
    nt = torch.full((B,), NKP, dtype=torch.int32, device=dev)
    qr = torch.full((B, M), RADIUS, dtype=torch.float32, device=dev)
    Pd = T(P)
    uvz = geometry.project_landmarks(X, nq, poses, Pd, W, H)
    grid = matcher.KeypointGrid(kp, nt, W, H, CELL)
    knn = matcher.window_knn2_batch(D, uvz[0], qr, nq, desc, kp, nt, grid)
    uni = matcher.unique_matches(*knn, nq, NKP)
    rows = matcher.track_rows(knn[0], uni[1], nq, kp, 0)
    torch.cuda.synchronize()
    steps = {
        "project": lambda: geometry.project_landmarks(X, nq, poses, Pd, W, H, out=uvz),
        "grid": lambda: grid.build(kp, nt),
        "window_knn2": lambda: matcher.window_knn2_batch(D, uvz[0], qr, nq, desc, kp, nt, grid, out=knn),
        "unique": lambda: matcher.unique_matches(*knn, nq, NKP, out=uni),
        "track_rows": lambda: matcher.track_rows(knn[0], uni[1], nq, kp, 0, out=rows),
    }
    res = {"M": M, "batch": B, "n_kp": NKP, "radius": RADIUS, "cell": CELL,
           "us": {k: round(timed(f), 2) for k, f in steps.items()}}
    chain = lambda names: (lambda: [steps[n]() for n in names])  # noqa: E731
    res["us"]["steps_2_4"] = round(timed(chain(["grid", "window_knn2", "unique"])), 2)
    res["us"]["steps_1_5"] = round(timed(chain(list(steps))), 2)
    valid = torch.isfinite(uvz[0][..., 0])
    res["visible_per_frame"] = round(float(valid.sum()) / B, 1)
    res["good_per_frame"] = round(float(knn[2].sum()) / B, 1)
    res["matched_per_frame"] = round(float(rows[1].sum()) / B, 1)
    # candidates a query reads: keypoints inside the windows, from the grid-independent definition
    k0, u0 = kp[0, :, :2], uvz[0][0][valid[0]][:4096]
    inside = ((k0[None, :, 0] - u0[:, None, 0]).abs() <= RADIUS) & ((k0[None, :, 1] - u0[:, None, 1]).abs() <= RADIUS)
    res["candidates_per_visible_query"] = round(float(inside.sum()) / max(len(u0), 1), 2)
    return res


def brute(rng):
    q = T(rng.integers(0, 256, (B, 2048, 32), dtype=np.uint8))
    t = T(rng.integers(0, 256, (B, NKP, 32), dtype=np.uint8))
    nq = torch.full((B,), 2048, dtype=torch.int32, device=q.device)
    nt = torch.full((B,), NKP, dtype=torch.int32, device=q.device)
    out = matcher.knn2_batch(q, nq, t, nt)
    us = timed(lambda: matcher.knn2_batch(q, nq, t, nt, out=out))
    return {"brute_force_knn2_us": round(us, 2), "q": 2048, "t": NKP, "batch": B,
            "gpairs_per_s": round(B * 2048 * NKP / us * 1e-3, 1)}


if __name__ == "__main__":
    rng = np.random.default_rng(7)
    sizes = [int(a) for a in sys.argv[1:]] or [2048, 65536]
    print(json.dumps(brute(rng)), flush=True)
    for M in sizes:
        print(json.dumps(measure(M, rng)), flush=True)
    print(json.dumps(brute(rng)), flush=True)
