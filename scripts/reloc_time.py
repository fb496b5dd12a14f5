"""Relocalization beside what it is measured against, in one process: the
global matcher slam_hamming_map_knn2 next to slam_hamming_knn2 on the same
sizes (2,048 keypoints per frame against 65,535 landmarks, the largest train set
slam_hamming_knn2 accepts, replicated per item for it), and the whole
LandmarkMap.relocalize next to LandmarkMap.localize on the same frames, at batch
1 and batch 32 -- HIP-event time per call (200 back-to-back calls, median of 5;
the two matchers alternate, two rounds each).  One JSON line per batch size.

The bars: at batch 1 the segmented kernel must be faster than the yardstick
(which launches 16 workgroups there), at batch 32 it may take at most 1.25 x
the yardstick's time.  Exit status 1 when one is missed.

    python scripts/reloc_time.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slam-1_amd"), os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from slam355 import matcher  # noqa: E402
from slam355.mapping import LandmarkMap  # noqa: E402

import guided_time as gt  # noqa: E402  (its scene, timer and camera: W, H, P)

M, NKP = 65535, 2048
T = gt.T


def measure(B, scene):
    X, D, poses, kp, desc = scene
    poses, kp, desc = T(poses[:B]), T(kp[:B, :NKP]), T(desc[:B, :NKP])
    dev = kp.device
    lm = LandmarkMap(M, NKP, gt.W, gt.H, gt.P, cell=gt.CELL).add(X, D)
    nq = torch.full((B,), NKP, dtype=torch.int32, device=dev)
    nt = torch.full((B,), M, dtype=torch.int32, device=dev)
    train = lm.desc[None].expand(B, M, 32).contiguous()           # the yardstick's train set per item
    rng = torch.tensor([[-(1 << 31), (1 << 31) - 1]] * B, dtype=torch.int32, device=dev)
    ws = matcher.map_knn2_workspace(B, NKP, M, dev)
    old = matcher.knn2_batch(desc, nq, train, nt)
    new = matcher.map_knn2_batch(desc, nq, lm.desc, lm.X, lm.last, lm.n_dev, rng, ws=ws)
    torch.cuda.synchronize()
    # the same neighbours: every landmark is alive and in range, so only the ratio test's max_dist differs
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])

    def yardstick():
        matcher.knn2_batch(desc, nq, train, nt, out=old)

    def segmented():
        matcher.map_knn2_batch(desc, nq, lm.desc, lm.X, lm.last, lm.n_dev, rng, ws=ws, out=new)

    us = {"knn2": [], "map_knn2": []}
    for _ in range(2):
        us["knn2"].append(gt.timed(yardstick))
        us["map_knn2"].append(gt.timed(segmented))
    lm.localize(0, poses, kp, desc, nq)
    lm.relocalize(0, kp, desc, nq)
    lm.reset_tracks()
    torch.cuda.synchronize()
    status = {"localize": lm.localize(0, poses, kp, desc, nq)[5].cpu().tolist(),
              "relocalize": lm.relocalize(0, kp, desc, nq)[5].cpu().tolist()}

    def localize():
        lm.localize(0, poses, kp, desc, nq)
        lm.reset_tracks()

    chain = {"localize": gt.timed(localize), "relocalize": gt.timed(lambda: lm.relocalize(0, kp, desc, nq))}
    ratio = min(us["map_knn2"]) / min(us["knn2"])
    ok = ratio < 1.0 if B == 1 else ratio <= 1.25
    print(json.dumps({
        "what": "reloc", "batch": B, "landmarks": M, "n_kp": NKP, "segment": matcher.MAP_KNN_SEGMENT,
        "knn2_us": [round(v, 2) for v in us["knn2"]], "map_knn2_us": [round(v, 2) for v in us["map_knn2"]],
        "map_over_knn2": round(ratio, 3), "bar": "< 1" if B == 1 else "<= 1.25", "bar_met": bool(ok),
        "gpairs_per_s": round(B * NKP * M / min(us["map_knn2"]) * 1e-3, 1),
        "chain_us": {k: round(v, 2) for k, v in chain.items()},
        "frames_status_0": {k: int(sum(1 for v in s if v == 0)) for k, s in status.items()}}), flush=True)
    return ok


def main():
    scene = gt.scene(M, np.random.default_rng(7))
    ok = [measure(B, scene) for B in (1, 32)]
    return 0 if all(ok) else 1


if __name__ == "__main__":
    sys.exit(main())
