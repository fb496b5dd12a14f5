"""Phase timing of k_solve_blk (needs a library built with -DSLAM_SOLVE_PROFILE:
`make -C slam-1_amd clean all HIPFLAGS_EXTRA=-DSLAM_SOLVE_PROFILE`)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slam-1_amd")]

from slam355 import _lib  # noqa: E402
from slam355.ba import BAProblem  # noqa: E402
from slam355.synthetic import ba_problem, perturb  # noqa: E402

# k_assemble launch (0) and k_solve_blk<true> (2: fused whatever the row count;
# its assembly prologue is a part of "load"), 16 chunks per supergroup as the
# tracker's windows and the planner's default
for C, P, k in ((6, 1500, 4), (10, 5000, 6), (13, 5000, 6)):
    for cpw in (16, None):
        for fused in (0, 2):
            _lib.call("slam_ba_set_fused_assembly", fused)
            rng = np.random.default_rng(0)
            cams, pts, ci, pi, qs = ba_problem(rng, C, P, k)
            c0, p0 = perturb(rng, cams, pts)
            prob = BAProblem(c0, p0, ci, pi, qs, chunks_per_wg=cpw)
            rows = []
            for _ in range(20):
                prob.iterate(1)
                rows.append(prob.t["state"][12:18].cpu().numpy())
            m = np.median(np.array(rows), 0)
            print(f"C={C} n={9 * C} chunks_per_wg={cpw} rows={prob._s.n_cslots + prob._s.n_bslots} "
                  f"fused={fused}: load {m[0]:.0f} ns (assembly prologue {m[5]:.0f} ns)  "
                  f"eliminate {m[1]:.0f} ns ({m[1] / (9 * C):.0f}/step)  backsub {m[2]:.0f} ns  "
                  f"epilogue {m[3]:.0f} ns")
_lib.call("slam_ba_set_fused_assembly", 1)
