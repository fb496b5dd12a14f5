"""Structure-only refinement (slam_points_refine) at a map's working size:
20,000 live landmarks in a capacity of 65,536, a window of 32 frames with up to
2,016 track rows each (every landmark seen in 2-5 consecutive frames, +-0.5 px of
noise, 3 % gross outliers, points 2 % of their depth off), default options.
slam_pose_refine on the same 32 frames, rows and map is the yardstick.  The two
calls alternate, X restored before every points call; HIP events round REPS
back-to-back calls, median of 5, launches included.  One JSON line.

    python scripts/points_refine_time.py
    rocprofv3 --kernel-trace --stats -d DIR -o points -- python scripts/points_refine_time.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slam-1_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from slam355 import geometry  # noqa: E402

F, ROWS_CAP, N, CAP = 32, 2016, 20000, 65536
W, H = 1280, 720
P = np.array([[700.0, 0, 640.0, 0], [0, 700.0, 360.0, 0], [0, 0, 1.0, 0]])
WARM, REPS = 20, 100


def scene(rng):
    poses = np.tile(np.eye(4), (F, 1, 1))
    for f in range(F):
        c, s = np.cos(0.01 * f), np.sin(0.01 * f)
        poses[f, :3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        poses[f, :3, 3] = [0.5 * f, 0.0, 0.1 * f]
    start = rng.integers(0, F, N)
    length = rng.integers(2, 6, N)
    z = rng.uniform(8.0, 40.0, N)
    X = np.stack([0.5 * start + rng.uniform(-0.5, 0.5, N) * z, rng.uniform(-0.3, 0.3, N) * z, z], 1)
    rows = np.zeros((F, ROWS_CAP, 4))
    count = np.zeros(F, np.int32)
    for f in range(F):
        ids = np.nonzero((start <= f) & (f < start + length))[0][:ROWS_CAP]
        Xc = (X[ids] - poses[f, :3, 3]) @ poses[f, :3, :3]
        uv = Xc[:, :2] / Xc[:, 2:] * 700.0 + (640.0, 360.0) + rng.uniform(-0.5, 0.5, (len(ids), 2))
        out = rng.random(len(ids)) < 0.03
        uv[out] += rng.uniform(30, 150, (int(out.sum()), 1)) * np.sign(rng.normal(0, 1, (int(out.sum()), 2)))
        rows[f, :len(ids)] = np.c_[np.full(len(ids), f), ids, uv]
        count[f] = len(ids)
    X0 = np.zeros((CAP, 3))
    X0[:N] = X + rng.normal(0, 0.02, (N, 3)) * z[:, None]
    pred = poses.copy()
    pred[:, :3, 3] += rng.normal(0, 0.05, (F, 3))
    return rows, count, poses, pred, X0


def timed(fn):
    torch.cuda.synchronize()
    t = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b) * 1e3 / REPS)
    return float(np.median(t))


if __name__ == "__main__":
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    rows, count, poses, pred, X0 = map(dev, scene(np.random.default_rng(11)))
    Pd, n_dev, X = dev(P), dev(np.array([N], np.int32)), X0.clone()
    ws = geometry.points_workspace(F, CAP)
    out = geometry.refine_points(rows, count, poses, Pd, X, n_dev, workspace=ws)
    pout = geometry.refine_pose(rows, count, X0, N, pred, Pd)

    def points():
        X.copy_(X0)
        geometry.refine_points(rows, count, poses, Pd, X, n_dev, out=out, workspace=ws)

    def pose():
        geometry.refine_pose(rows, count, X0, N, pred, Pd, out=pout)

    for _ in range(WARM):
        points()
        pose()
    t_points, t_pose = timed(points), timed(pose)
    t_points2, t_pose2 = timed(points), timed(pose)
    t_copy = timed(lambda: X.copy_(X0))
    points()
    torch.cuda.synchronize()
    st = out[0][:N].cpu().numpy()
    print(json.dumps({
        "what": "refine_points", "frames": F, "rows_cap": ROWS_CAP, "landmarks": N, "capacity": CAP,
        "rows": int(count.sum()), "status_histogram": [int((st == k).sum()) for k in range(5)],
        "points_us_per_call": [round(t_points - t_copy, 2), round(t_points2 - t_copy, 2)],
        "restore_X_us": round(t_copy, 2),
        "pose_refine_us_per_call": [round(t_pose, 2), round(t_pose2, 2)],
        "pose_status_ok": int((pout[3] == 0).sum())}), flush=True)
