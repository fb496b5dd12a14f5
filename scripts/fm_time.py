"""F-LMedS alone on the tracking batch shape (64 frame pairs x ~600 stereo
matches, 15 % outliers, 300 hypotheses): mean ms per call, for A/B of the
hypothesis kernels (run under rocprofv3 --kernel-trace --stats for the
per-kernel split).  With a -DSLAM_FMH_TRACE library it also prints the FMH_T
stamps of workgroup (3, 5) of the scoring kernel as s_memtime ticks and shares
of the workgroup's life (0: start, 1: candidates / points ready, 2: scored,
3: merged).

    python scripts/fm_time.py [LIB_NAME]   (slam-1_amd/prof/libslam355_LIB_NAME.so)"""
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slam-1_amd")]
if len(sys.argv) > 1:
    os.environ["SLAM355_LIB"] = os.path.join(ROOT, "slam-1_amd", "prof", f"libslam355_{sys.argv[1]}.so")

import torch  # noqa: E402
from slam355 import _lib, geometry  # noqa: E402

B, cap, N_HYP = 64, 2112, 300
rng = np.random.default_rng(0)
m1 = np.zeros((B, cap, 2))
m2 = np.zeros((B, cap, 2))
cnt = np.zeros(B, np.int32)
f, cx, cy, base = 718.856, 640.0, 360.0, 0.54
for b in range(B):
    n = int(rng.integers(560, 650))
    X = np.c_[rng.uniform(-10, 10, n), rng.uniform(-3, 3, n), rng.uniform(5, 60, n)]
    pl = X[:, :2] / X[:, 2:] * f + [cx, cy] + rng.normal(0, 0.4, (n, 2))
    Xr = X - [base, 0, 0]
    pr = Xr[:, :2] / Xr[:, 2:] * f + [cx, cy] + rng.normal(0, 0.4, (n, 2))
    out = rng.random(n) < 0.15
    pr[out] = rng.uniform([0, 0], [1280, 720], (int(out.sum()), 2))
    m1[b, :n], m2[b, :n], cnt[b] = pl, pr, n
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
t1, t2, tc = T(m1), T(m2), T(cnt)
ws = geometry.fundamental_workspace(B, N_HYP)
for i in range(3):
    geometry.fundamental_lmeds(t1, t2, tc, seed=1, item0=i, n_hyp=N_HYP, ws=ws)
torch.cuda.synchronize()
N = 20
t0 = time.perf_counter()
for i in range(N):
    mask, F, ninl = geometry.fundamental_lmeds(t1, t2, tc, seed=1, item0=i, n_hyp=N_HYP, ws=ws)
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) / N * 1e3
print(f"fundamental_lmeds B={B} M~600 n_hyp={N_HYP}: {ms:.3f} ms per call; "
      f"inliers mean {ninl.float().mean().item():.1f}")
if hasattr(_lib.lib, "slam_fmh_trace"):
    buf = (ctypes.c_ulonglong * 8)()
    fn = _lib.lib.slam_fmh_trace
    fn.argtypes = [ctypes.c_void_p]
    _lib.check(fn(buf), "slam_fmh_trace")
    v = list(buf)
    d = [v[1] - v[0], v[2] - v[1], v[3] - v[2]]
    tot = max(sum(d), 1)
    print(f"FMH_T ticks 0-1 / 1-2 / 2-3: {d[0]} / {d[1]} / {d[2]} "
          f"({100 * d[0] / tot:.1f} / {100 * d[1] / tot:.1f} / {100 * d[2] / tot:.1f} % of {tot}); "
          f"wave 0: {v[5]} candidates, {v[6]} median selects, M {v[7]}")
