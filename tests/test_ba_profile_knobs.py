"""Every profiling knob of the BA translation unit still compiles.

csrc/ba.hip keeps four profiling builds,
each with a reader under scripts/: -DSLAM_SOLVE_PROFILE (ba_solve_prof.py),
-DSLAM_SOLVE_TRACE (solve_trace.py), -DSLAM_LINM_PROFILE (linm_prof.py) and
-DSLAM_FLOW_PROFILE (flow_prof.py).  The default build never sees the code
behind them, so a knob can stop compiling unnoticed; this runs the compiler's
front end (host and gfx950 passes, no code generation) over the file with
each knob alone and with all four together.  No GPU, no library.
"""
import os
import re
import subprocess

import pytest

from conftest import ROOT

KNOBS = ["SLAM_SOLVE_PROFILE", "SLAM_SOLVE_TRACE", "SLAM_LINM_PROFILE", "SLAM_FLOW_PROFILE"]
AMD = os.path.join(ROOT, "slam-1_amd")


def _hipcc():
    """The Makefile's compiler: its `HIPCC ?=` default unless the environment sets one."""
    mk = open(os.path.join(AMD, "Makefile")).read()
    return os.environ.get("HIPCC") or re.search(r"^HIPCC \?= *(\S+)", mk, flags=re.M).group(1)


@pytest.mark.parametrize("knobs", [[k] for k in KNOBS] + [KNOBS], ids=lambda ks: "+".join(ks))
def test_ba_compiles_with_profiling_knob(knobs):
    cmd = [_hipcc(), "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only"]
    cmd += ["-D" + k for k in knobs] + ["csrc/ba.hip"]
    r = subprocess.run(cmd, cwd=AMD, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]
