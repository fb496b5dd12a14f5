"""Golden fixtures that pin the PnP hypothesis kernels (k_pnp_hyp, k_pnp_hyp_lm)
and what k_pnp makes of their poses, bit for bit, to the commit they were
generated at (run once on the GPU, before a kernel of that chain changes):

    python tests/golden/make_pnp_hyp_goldens.py [OUT.npz]

One batch of five items, cap 48, rows past each count filled with NaN (a row
that is read shows up as a NaN in the results):
    count  5   the minimum: every sample is the same five points
    count 37   generic, 20 % outliers
    count  4   the L < 5 guard: ninliers -1, its workspace rows never written
    count 12   all points coincident: every sample degenerate (ep_bary returns
               0), LM from r = t = 0
    count 48   large rotation
For each n_hyp of N_HYP (the default; 6: no multiple of the hypotheses a
workgroup of either kernel holds; 1) it stores the workspace after
pnp_ransac(hyp_iters=0) (the EPnP poses), the workspace after hyp_iters=10,
and rvec, tvec, ninliers, mask of that second call.  The workspace is filled
with NaN before each call, so rows no kernel writes compare equal as well.
Only data (inputs + outputs) is written.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slam-1_amd")]

COUNTS = (5, 37, 4, 12, 48)
CAP = 48
N_HYP = (100, 6, 1)
SEED, ITEM0 = 21, 300


def _rodrigues(r):
    th = np.linalg.norm(r)
    k = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]]) / th
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * k @ k


def inputs():
    K = np.array([[718.856, 0, 607.19], [0, 718.856, 185.22], [0, 0, 1]])
    rng = np.random.default_rng(48)
    B = len(COUNTS)
    Q = np.full((B, CAP, 3), np.nan)
    q = np.full((B, CAP, 2), np.nan)
    rvecs = ([0.01, -0.02, 0.005], [0.02, 0.05, -0.01], [0.0, 0.01, 0.0], [0.01, 0.0, 0.0],
             [0.9, -1.4, 0.6])  # the last: |r| = 1.77 rad
    for b, n in enumerate(COUNTS):
        X = np.stack([rng.uniform(-8, 8, n), rng.uniform(-3, 3, n), rng.uniform(6, 40, n)], 1)
        if n == 12:
            X[:] = X[0]
        if b == 4:  # keep the rotated points in front of the camera
            X = X - X.mean(0)
            t = np.array([0.3, -0.2, 25.0])
        else:
            t = np.array([0.05, -0.02, -0.8])
        Xc = X @ _rodrigues(np.array(rvecs[b])).T + t
        uv = Xc[:, :2] / Xc[:, 2:3] * [K[0, 0], K[1, 1]] + K[:2, 2] + rng.normal(0, 0.5, (n, 2))
        if n == 12:
            uv[:] = uv[0]
        if n == 37:
            k = int(0.2 * n)
            uv[:k] += rng.uniform(-120, 120, (k, 2))
        Q[b, :n], q[b, :n] = X, uv
    return Q, q, np.array(COUNTS, np.int32), K


def run(Q, q, cnt, K, n_hyp, hyp_iters, **kw):
    """(ws, rvec, tvec, ninliers, mask) of one pnp_ransac call, as numpy."""
    import torch
    from slam355 import geometry

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    ws = torch.full((len(cnt) * n_hyp * 6,), float("nan"), dtype=torch.float64, device="cuda")
    out = geometry.pnp_ransac(T(Q), T(q), T(cnt), K, seed=SEED, item0=ITEM0, n_hyp=n_hyp,
                              hyp_iters=hyp_iters, ws=ws, **kw)
    torch.cuda.synchronize()
    return (ws.cpu().numpy(),) + tuple(x.cpu().numpy() for x in out)


def main():
    Q, q, cnt, K = inputs()
    g = dict(Q=Q, q=q, count=cnt, K=K)
    for n_hyp in N_HYP:
        g[f"ws0_{n_hyp}"] = run(Q, q, cnt, K, n_hyp, 0)[0]
        ws, rv, tv, n, mask = run(Q, q, cnt, K, n_hyp, 10)
        for k, v in dict(ws10=ws, rvec=rv, tvec=tv, ninliers=n, mask=mask).items():
            g[f"{k}_{n_hyp}"] = v
        print(n_hyp, "ninliers", n.tolist(), "NaN in ws0 / ws10",
              int(np.isnan(g[f"ws0_{n_hyp}"]).sum()), int(np.isnan(ws).sum()),
              "zero EPnP poses", int((g[f"ws0_{n_hyp}"].reshape(-1, 6) == 0).all(1).sum()))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "pnp_hyp_golden.npz")
    np.savez_compressed(out, **g)


if __name__ == "__main__":
    main()
