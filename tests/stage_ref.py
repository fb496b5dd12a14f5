"""Mapper-shaped inputs of BAWindowSet.stage / slam_ba_stage_windows for the
window-set tests (test_ba.py, test_ba_fixed.py, test_ba_loss.py)."""
import numpy as np


def synthetic_windows(specs, n, seed):
    """Perturbed synthetic windows of n cameras, one per (P, k) of specs:
    [(cams, pts, cam_idx, pt_idx, qs), ...]."""
    from slam355.synthetic import ba_problem, perturb

    wins = []
    for w, (P, k) in enumerate(specs):
        rng = np.random.default_rng(seed + w)
        cams, pts, ci, pi, qs = ba_problem(rng, n, P, k)
        wins.append((*perturb(rng, cams, pts), ci, pi, qs))
    return wins


def stage_inputs(wins, n, u_off=0.5, v_off=0.25):
    """Mapper-shaped host arrays (rows [W n, cap, 4] = (frame, point, u, v),
    counts, maps, M, cams) for windows of n cameras, each window's
    observations dealt over its n pairs in order, and the problems they stand
    for (q = u - u_off: the stager's arithmetic)."""
    W = len(wins)
    cap = max(-(-len(w[2]) // n) for w in wins)
    rows = np.zeros((W * n, cap, 4))
    cnt = np.zeros(W * n, np.int32)
    maps = np.zeros((W, max(len(w[1]) for w in wins), 3))
    M = np.zeros(W, np.int32)
    cams = np.zeros((W * n, 9))
    probs = []
    for w, (c0, p0, ci, pi, qs) in enumerate(wins):
        maps[w, :len(p0)] = p0
        M[w] = len(p0)
        cams[w * n:(w + 1) * n] = c0
        qq = []
        for j, idx in enumerate(np.array_split(np.arange(len(ci)), n)):
            b = w * n + j
            cnt[b] = len(idx)
            rows[b, :len(idx)] = np.stack([ci[idx], pi[idx], qs[idx, 0] + u_off, qs[idx, 1] + v_off], 1)
            qq.append(np.stack([rows[b, :len(idx), 2] - u_off, rows[b, :len(idx), 3] - v_off], 1))
        probs.append((c0, p0, ci, pi, np.concatenate(qq)))
    return (rows, cnt, maps, M, cams, u_off, v_off), probs
