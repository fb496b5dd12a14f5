"""Time per BAProblem.point_covariance() call (profiles/ba_ptcov/).

    python scripts/ba_ptcov_time.py c3|c4

HIP events, median of 5 calls after one warm-up, device=True (no copy of the
results to the host inside the timed region; the request lists are uploaded
inside it, as in every call).  Set-up of scripts/ba_cov_time.py: cameras 0 and
1 held whole, 10 LM iterations from the perturbed start.  One JSON line:
  covariance_ms        covariance(): every camera's own block
  point_all_ms         point_covariance(): every point + the same camera blocks
  point_1000_ms        the same with 1000 points instead of all
  cross_1000_ms        1000 (point, camera) blocks + the same camera blocks
  marked_pairs_ms      covariance() with every camera pair (a, b), |a - b| < 6, added: the
                       tiles an all-points request marks, without the contraction
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "slam-1_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from slam355 import ba  # noqa: E402
from slam355.synthetic import ba_problem, perturb  # noqa: E402

SHAPES = {"c3": (10, 5000, 6), "c4": (64, 50000, 6)}


def timed(fn, reps=5):
    fn()  # warm-up
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(float(np.median(ms)), 3), [round(m, 3) for m in ms]


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "c3"
    C, P, k = SHAPES[name]
    rng = np.random.default_rng(7)
    cams, pts, ci, pi, qs = ba_problem(rng, C, P, k)
    c0, p0 = perturb(rng, cams, pts)
    fx = np.zeros((C, 9), np.uint8)
    fx[:2] = 1
    prob = ba.BAProblem(c0, p0, ci, pi, qs, fixed=fx)
    prob.iterate(10)
    torch.cuda.synchronize()
    allc = np.arange(C)
    some = np.random.default_rng(1).integers(0, P, 1000)
    cross = np.stack([some, np.random.default_rng(2).integers(0, C, 1000)], 1)
    near = [(a, b) for a in range(C) for b in range(C) if a != b and abs(a - b) < k]
    rec = {"shape": name, "C": C, "P": P, "O": int(len(ci)), "tiles": -(-9 * C // 64), "lin_mode": prob.lin_mode}
    for key, fn in (("covariance_ms", lambda: prob.covariance(device=True)),
                    ("point_all_ms", lambda: prob.point_covariance(cameras=allc, device=True)),
                    ("point_1000_ms", lambda: prob.point_covariance(points=some, cameras=allc, device=True)),
                    ("cross_1000_ms", lambda: prob.point_covariance(points=[], cross=cross, cameras=allc, device=True)),
                    ("marked_pairs_ms", lambda: prob.covariance(cameras=allc, pairs=near, device=True))):
        rec[key], rec[key + "_runs"] = timed(fn)
    rec["contraction_ms"] = round(rec["point_all_ms"] - rec["covariance_ms"], 3)
    rec["extra_tiles_ms"] = round(rec["marked_pairs_ms"] - rec["covariance_ms"], 3)
    out = prob.point_covariance(cameras=allc, device=True)
    torch.cuda.synchronize()
    rec["status"], rec["undetermined"] = prob.cov_status(), prob.cov_undetermined()
    rec["finite"] = bool(torch.isfinite(out.points).all())
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
