"""Time per BAProblem.covariance() call (profiles/ba_cov/).

    python scripts/ba_cov_time.py c3|c4|c5|c5open

HIP events, median of 5 calls after one warm-up, every marginal block
requested, device=True (no host copy inside the timed region).  The build
(slam_ba_build_system alone) is timed the same way; the inverse is the
difference.  Yardstick: torch.linalg.inv of the same dense S0 (held rows as
unit rows) on the same GPU.  One JSON line.

Shapes: c3 10 x 5000 x 6, c4 64 x 50000 x 6 (bench.py --c4), c5 500 x 200000 x 6
on the closed loop (bench.py --c5), c5open the same size on ba_problem's open
trajectory.  Cameras 0 and 1 are held whole; a few LM iterations run first.
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
from slam355.synthetic import ba_problem, ba_problem_loop, perturb  # noqa: E402

SHAPES = {"c3": (10, 5000, 6, ba_problem), "c4": (64, 50000, 6, ba_problem),
          "c5": (500, 200000, 6, ba_problem_loop), "c5open": (500, 200000, 6, ba_problem)}


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
    return float(np.median(ms)), [round(m, 3) for m in ms]


def dense_s0(prob):
    """S0 as covariance() left it in sys, held rows and columns as unit rows."""
    C, n = prob.C, 9 * prob.C
    sys_ = prob.t["sys"]
    if ba.packed(C):
        blk = torch.from_numpy(np.asarray(prob.plan["blocks"]).reshape(-1, 2).astype(np.int64)).cuda()
        v = sys_[:81 * len(blk)].view(-1, 9, 9)
        S = torch.zeros((C, 9, C, 9), dtype=torch.float64, device="cuda")
        S[blk[:, 0], :, blk[:, 1], :] = v
        off = blk[:, 0] != blk[:, 1]
        S[blk[off, 1], :, blk[off, 0], :] = v[off].transpose(1, 2)
        S = S.reshape(n, n).contiguous()
    else:
        S = sys_[:n * n].view(n, n).clone()
    held = torch.from_numpy(((prob.fixed[:, None] >> np.arange(9, dtype=np.uint32)) & 1).astype(bool).ravel()).cuda()
    S[held, :] = 0.0
    S[:, held] = 0.0
    S[held, held] = 1.0
    return S, held


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "c3"
    C, P, k, gen = SHAPES[name]
    rng = np.random.default_rng(7)
    cams, pts, ci, pi, qs = gen(rng, C, P, k)
    c0, p0 = perturb(rng, cams, pts)
    fx = np.zeros((C, 9), np.uint8)
    fx[:2] = 1
    prob = ba.BAProblem(c0, p0, ci, pi, qs, fixed=fx)
    prob.iterate(10)
    torch.cuda.synchronize()
    total, total_all = timed(lambda: prob.covariance(device=True))
    status = prob.cov_status()
    build, build_all = timed(prob.build_system)
    out = prob.covariance(device=True)
    S, held = dense_s0(prob)
    rec = {"shape": name, "C": C, "P": P, "O": int(len(ci)), "tiles": -(-9 * C // 64), "status": status,
           "covariance_ms": round(total, 3), "build_ms": round(build, 3), "inverse_ms": round(total - build, 3),
           "covariance_ms_runs": total_all, "build_ms_runs": build_all}
    # the same S0 inverted by the host's LAPACK: the correlation-scaled deviation
    # of the marginal blocks (and of torch's inverse) from it
    ref = np.linalg.inv(S.cpu().numpy())
    hm = ~held.cpu().numpy()
    d = np.sqrt(np.diag(ref))

    def deviation(blocks):
        worst = 0.0
        for a in range(C):
            sl = slice(9 * a, 9 * a + 9)
            m = hm[sl]
            if m.any():
                sc = np.outer(d[sl], d[sl])[np.ix_(m, m)]
                worst = max(worst, float(np.max(np.abs(blocks[a] - ref[sl, sl])[np.ix_(m, m)] / sc)))
        return worst

    if status == 0:
        rec["deviation_from_host_inv"] = deviation(out.cpu().numpy())
    if 9 * C <= 1000:
        rec["cond_s0"] = float(np.linalg.cond(S.cpu().numpy()))
    try:
        inv_ms, inv_all = timed(lambda: torch.linalg.inv(S))
        rec["torch_linalg_inv_ms"], rec["torch_linalg_inv_ms_runs"] = round(inv_ms, 3), inv_all
        Si = torch.linalg.inv(S).cpu().numpy()
        rec["torch_inv_deviation_from_host_inv"] = deviation([Si[9 * a:9 * a + 9, 9 * a:9 * a + 9] for a in range(C)])
    except Exception as e:  # noqa: BLE001 (the yardstick may not run on this build of torch)
        rec["torch_linalg_inv_ms"] = None
        rec["torch_linalg_inv_error"] = f"{type(e).__name__}: {e}"[:200]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
