"""Every profiling knob of the BA translation units still compiles.

The BA files (csrc/ba*.hip) keep four profiling builds,
each with a reader under scripts/: -DSLAM_SOLVE_PROFILE (ba_solve_prof.py),
-DSLAM_SOLVE_TRACE (solve_trace.py), -DSLAM_LINM_PROFILE (linm_prof.py) and
-DSLAM_FLOW_PROFILE (flow_prof.py).  The default build never sees the code
behind them, so a knob can stop compiling unnoticed; this runs the compiler's
front end (host and gfx950 passes, no code generation) over every BA file
with each knob alone and with all four together (a knob reaches the shared
headers, so every file sees it).  No GPU, no library.
"""
import glob
import os
import re
import subprocess

import pytest

from conftest import ROOT

KNOBS = ["SLAM_SOLVE_PROFILE", "SLAM_SOLVE_TRACE", "SLAM_LINM_PROFILE", "SLAM_FLOW_PROFILE"]
AMD = os.path.join(ROOT, "slam-1_amd")
FILES = sorted(os.path.relpath(f, AMD) for f in glob.glob(os.path.join(AMD, "csrc", "ba*.hip")))


def _hipcc():
    """The Makefile's compiler: its `HIPCC ?=` default unless the environment sets one."""
    mk = open(os.path.join(AMD, "Makefile")).read()
    return os.environ.get("HIPCC") or re.search(r"^HIPCC \?= *(\S+)", mk, flags=re.M).group(1)


def test_ba_files_found():
    assert "csrc/ba.hip" in FILES and len(FILES) >= 2, FILES


@pytest.mark.parametrize("knobs", [[k] for k in KNOBS] + [KNOBS], ids=lambda ks: "+".join(ks))
@pytest.mark.parametrize("src", FILES, ids=os.path.basename)
def test_ba_compiles_with_profiling_knob(src, knobs):
    cmd = [_hipcc(), "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only"]
    cmd += ["-D" + k for k in knobs] + [src]
    r = subprocess.run(cmd, cwd=AMD, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]
