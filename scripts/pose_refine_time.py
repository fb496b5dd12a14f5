"""Pose refinement (slam_pose_refine) on a tracking batch: 32 frames of N
observations each (30 % gross outliers, 1 px noise, predictions 0.1 m and
0.004 rad off), the defaults of 4 rounds x 10 LM iterations with the huber
loss -- HIP-event time per call with the launch in it, and per LM iteration.
Then a full LandmarkMap.localize (observe, refine, observe, refine) beside
observe alone at 2,048 landmarks and 2,087 keypoints per 1280 x 720 frame.
One JSON line per measurement.

    python scripts/pose_refine_time.py [N ...]     (default: 200 2000)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slam-1_amd"), os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from slam355 import geometry  # noqa: E402
from slam355.mapping import LandmarkMap  # noqa: E402

import guided_time as gt  # noqa: E402  (its scene, timer and shape: B, NKP, W, H, P)

B, ROUNDS_LM, ITERS = 32, 4, 10
T = gt.T


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def refine_scene(N, rng):
    rows = np.zeros((B, N, 4))
    pred = np.tile(np.eye(4), (B, 1, 1))
    Xs = []
    for b in range(B):
        R, t = rot(rng.normal(0, 1, 3), 0.05), rng.uniform(-1, 1, 3)
        z = rng.uniform(4, 40, N)
        Xc = np.stack([rng.uniform(-0.8, 0.8, N) * z, rng.uniform(-0.45, 0.45, N) * z, z], 1)
        uv = Xc[:, :2] / Xc[:, 2:] * 700.0 + (640.0, 360.0) + rng.uniform(-1, 1, (N, 2))
        out = rng.random(N) < 0.3
        uv[out] += rng.uniform(50, 200, (int(out.sum()), 1)) * np.sign(rng.normal(0, 1, (int(out.sum()), 2)))
        Xs.append(Xc @ R.T + t)
        rows[b] = np.c_[np.full(N, b), b * N + np.arange(N), uv]
        d = rng.normal(0, 1, 3)
        pred[b, :3, :3], pred[b, :3, 3] = R @ rot(rng.normal(0, 1, 3), 0.004), t + 0.1 * d / np.linalg.norm(d)
    return rows, np.concatenate(Xs), pred


def measure_refine(N, rng):
    rows, X, pred = map(T, refine_scene(N, rng))
    count = torch.full((B,), N, dtype=torch.int32, device=rows.device)
    Pd = T(gt.P)
    kw = dict(rounds=ROUNDS_LM, iters=ITERS)
    out = geometry.refine_pose(rows, count, X, X.shape[0], pred, Pd, **kw)
    us = gt.timed(lambda: geometry.refine_pose(rows, count, X, X.shape[0], pred, Pd, out=out, **kw))
    torch.cuda.synchronize()
    return {"what": "refine_pose", "batch": B, "obs_per_frame": N, "rounds": ROUNDS_LM, "iters": ITERS,
            "loss": "huber", "us_per_call": round(us, 2),
            "us_per_lm_iteration": round(us / (ROUNDS_LM * ITERS), 3),
            "status_ok": int((out[3] == 0).sum()), "inliers_per_frame": round(float(out[2].sum()) / B, 1)}


def measure_localize(M, rng):
    X, D, poses, kp, desc = gt.scene(M, rng)
    lm = LandmarkMap(M, gt.NKP, gt.W, gt.H, gt.P, cell=gt.CELL).add(X, D)
    poses, kp, desc = T(poses), T(kp), T(desc)
    nt = torch.full((B,), gt.NKP, dtype=torch.int32, device=kp.device)

    def observe():
        lm.observe(0, poses, kp, desc, nt, radius=15.0)
        lm.reset_tracks()

    def localize():
        res = lm.localize(0, poses, kp, desc, nt, radius=(15.0, 5.0), rounds=ROUNDS_LM, iters=ITERS)
        lm.reset_tracks()
        return res

    res = localize()
    torch.cuda.synchronize()
    return {"what": "localize", "M": M, "batch": B, "n_kp": gt.NKP, "radius": [15.0, 5.0],
            "observe_us": round(gt.timed(observe), 2), "localize_us": round(gt.timed(localize), 2),
            "observe_again_us": round(gt.timed(observe), 2),
            "status_ok": int((res[5] == 0).sum()), "rows_per_frame": round(float(res[2].sum()) / B, 1),
            "inliers_per_frame": round(float(res[4].sum()) / B, 1)}


if __name__ == "__main__":
    rng = np.random.default_rng(7)
    for N in [int(a) for a in sys.argv[1:]] or [200, 2000]:
        print(json.dumps(measure_refine(N, rng)), flush=True)
    print(json.dumps(measure_localize(2048, rng)), flush=True)
