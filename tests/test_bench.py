"""bench.py's own contract: what a plain run measures, what --full adds, and what
--dump-outputs writes.

CPU: dump_outputs (types, the byte budget, the fixed sample of an oversized array).
GPU: one small tracking run per mode as a child process (the command line is what
is under test): the plain line carries the headline fields and none of the side
measurements, --steps sets the timed steps, the dumped poses are the ones the
line's trajectory_sha1 hashes; --full brings the side measurements back.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "8", "--windows", "2",
         "--ba-group", "1"]
SIDE = ("pcie_inclusive", "tracked_source", "tracked_window_ba", "local_ba_sharded", "cpu_baseline")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_dump_outputs_types_budget_and_fixed_sample(tmp_path, monkeypatch):
    import bench

    rng = np.random.default_rng(1)
    arrays = {"counts": np.arange(5, dtype=np.int32), "bytes": rng.integers(0, 256, (4, 32), np.uint8),
              "single": rng.normal(size=(3, 3)).astype(np.float32), "big": rng.normal(size=(100, 100))}
    monkeypatch.setattr(bench, "DUMP_BUDGET", 8192)
    shapes = [bench.dump_outputs(str(tmp_path / d), arrays) for d in ("a", "b")]
    assert shapes[0] == shapes[1] and set(shapes[0]) == set(arrays)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in arrays}
    assert got["counts"].dtype == np.float64 and np.array_equal(got["counts"], arrays["counts"])
    assert got["bytes"].dtype == np.float32 and np.array_equal(got["bytes"], arrays["bytes"])
    assert got["single"].dtype == np.float32 and np.array_equal(got["single"], arrays["single"])
    # the oversized array: a sorted, seeded sample of its flat elements, the same in both runs
    big = got["big"]
    assert big.dtype == np.float64 and big.ndim == 1 and 0 < big.size < arrays["big"].size
    idx = np.sort(np.random.default_rng(0).choice(arrays["big"].size, big.size, replace=False))
    assert np.array_equal(big, arrays["big"].ravel()[idx])
    assert np.array_equal(big, np.load(tmp_path / "b" / "big.npy"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 8192


@pytest.mark.gpu
def test_gpu_plain_run_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    out = tmp_path / "dump"
    rec = _bench("--dump-outputs", str(out))
    assert rec["metric"] == "frames/sec tracking+local-BA @1280x720" and rec["unit"] == "frames/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "u8+f32+f64" and rec["full"] is False
    assert rec["steps"] == 2 and len(rec["host_issue_ms_per_step_list"]) == 2
    # value = frames of the timed steps / their time; ms_per_step = that time / steps
    assert rec["ms_per_step"] > 0 and np.isclose(rec["value"], 8 / (rec["ms_per_step"] * 1e-3), rtol=1e-9)
    assert not [k for k in SIDE if k in rec]
    files = sorted(os.listdir(out))
    assert files == sorted(n + ".npy" for n in rec["dumped_outputs"])
    assert sum(os.path.getsize(out / f) for f in files) <= 64e6
    arr = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arr.values())
    assert arr["poses"].shape == (8, 4, 4) and arr["rvec"].shape == (8, 3)
    assert hashlib.sha1(arr["poses"].tobytes()).hexdigest() == rec["tracking"]["trajectory_sha1"]
    assert (arr["pnp_inliers"] > 0).all() and np.isfinite(arr["poses"]).all()
    # rows past each image's keypoint count are zeroed, rows below it are keypoints
    kp, n = arr["orb_keypoints"], arr["orb_count"].astype(int)
    assert kp.shape[0] == 17 and (n > 0).all()
    assert all(kp[i, :n[i], 2].all() and not kp[i, n[i]:].any() for i in range(17))
    assert arr["ba_cams"].shape == (1, 10, 9) and arr["ba_points"].shape == (1, 5000, 3)
    assert arr["ba_cost"].shape == (1,) and np.isfinite(arr["ba_cost"]).all()


@pytest.mark.gpu
def test_gpu_full_run_adds_the_side_measurements():
    rec = _bench("--full", "--no-cpu-baseline", "--no-ba-scale")
    assert rec["full"] is True and rec["steps"] == 2
    for k in ("pcie_inclusive", "tracked_source", "tracked_window_ba"):
        assert k in rec, k
    assert rec["pcie_inclusive"]["ms_per_step"] > 0 and rec["tracked_source"]["frames_per_s"] > 0
