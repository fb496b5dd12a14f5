"""Landmark life cycle (LandmarkMap.score / spawn / cull / compact) beside
LandmarkMap.observe in the same process: batch 32, 65,536 landmarks in view,
2,087 keypoints per 1280 x 720 frame, 8 keyframes with 300 spawn candidates
each -- HIP-event time per call with the launches in it (200 back-to-back
calls, median of 5).  One JSON line.

A spawn changes what the next spawn sees (the keypoints it took are owned, the
count has grown), so every timed spawn is preceded by putting `owner` and the
count back; that restore is timed alone as well, and the bar uses the spawn
WITH its restore.  The timed cull reads and tests every landmark with
thresholds nobody meets (a cull that kills changes the map under the other
measurements); one real cull by age follows, and compact is timed on its result.

    python scripts/map_life_time.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slam-1_amd"), os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from slam355 import _lib  # noqa: E402
from slam355.device import ptr  # noqa: E402
from slam355.mapping import LandmarkMap  # noqa: E402

import guided_time as gt  # noqa: E402  (its scene, timer and shape: B, NKP, W, H, P)

M, KEYFRAMES, CANDIDATES = 65536, 8, 300
B, T = gt.B, gt.T


def main():
    rng = np.random.default_rng(7)
    X, D, poses, kp, desc = gt.scene(M, rng)
    cap = M + KEYFRAMES * CANDIDATES
    lm = LandmarkMap(cap, gt.NKP, gt.W, gt.H, gt.P, cell=gt.CELL).add(X, D)
    poses, kp, desc = T(poses), T(kp), T(desc)
    nt = torch.full((B,), gt.NKP, dtype=torch.int32, device=kp.device)

    def observe():
        out = lm.observe(0, poses, kp, desc, nt, radius=gt.RADIUS)
        lm.reset_tracks()
        return out

    rows, count = observe()
    torch.cuda.synchronize()
    visible = float(torch.isfinite(lm.uv[..., 0]).sum()) / B
    matched = float(count.sum()) / B
    # stereo pairs: every keypoint once, in random order; exactly CANDIDATES of the
    # unowned ones carry a point in the depth range, the rest lie beyond it
    owner = lm.owner.cpu().numpy()
    keyframe = np.zeros(B, np.uint8)
    keyframe[B // KEYFRAMES - 1::B // KEYFRAMES] = 1
    pairs = np.zeros((B, gt.NKP, 2), np.int32)
    z = np.full((B, gt.NKP), 500.0)
    for b in range(B):
        order = rng.permutation(gt.NKP)
        pairs[b, :, 0] = pairs[b, :, 1] = order
        free = np.nonzero(owner[b, order] == -1)[0]
        assert len(free) >= CANDIDATES
        z[b, rng.permutation(free)[:CANDIDATES]] = rng.uniform(4, 40, CANDIDATES)
    Xc = np.stack([rng.uniform(-0.9, 0.9, z.shape) * z, rng.uniform(-0.5, 0.5, z.shape) * z, z], 2)
    Xc, pairs, keyframe = T(Xc), T(pairs), T(keyframe)
    owner0, count0 = lm.owner.clone(), count.clone()

    def restore():
        lm.owner.copy_(owner0)
        count.copy_(count0)
        lm.n_dev.fill_(M)

    def spawn():
        restore()
        return lm.spawn(0, poses, Xc, pairs, nt, kp, desc, nt, keyframe, rows=rows, rows_count=count)

    spawned, dropped = spawn()
    torch.cuda.synchronize()
    assert int(dropped.item()) == 0 and spawned.cpu().tolist() == [CANDIDATES * int(k) for k in keyframe.cpu()]
    never = dict(min_visible=1 << 30, age=1 << 30)
    us = {"observe": gt.timed(observe), "score": gt.timed(lambda: lm.score(0)),
          "spawn_with_restore": gt.timed(spawn), "restore": gt.timed(restore),
          "cull": gt.timed(lambda: lm.cull(B - 1, **never))}
    us["observe_again"] = gt.timed(observe)
    assert int(lm.nculled.item()) == 0
    # one real cull, then compact from it (the age rule alone: every frame of this scene shows a
    # random 1 in 40 of the landmarks, which the ratio rule would not forgive)
    died = int(lm.cull(B - 1, ratio=(0, 1)).item())
    lm.compact()
    src, dst = lm._alt, lm._fields()              # the map as culled, and somewhere to put it
    n_src = torch.tensor([M + KEYFRAMES * CANDIDATES], dtype=torch.int32, device=kp.device)
    n_out = torch.zeros_like(n_src)

    def compact():
        _lib.call("slam_map_compact", *(ptr(t) for t in src), ptr(n_src), cap, *(ptr(t) for t in dst),
                  ptr(lm.remap), ptr(n_out), None)

    us["compact"] = gt.timed(compact)
    torch.cuda.synchronize()
    cycle = us["score"] + us["spawn_with_restore"] + us["cull"]
    print(json.dumps({
        "what": "map_life", "landmarks": M, "batch": B, "n_kp": gt.NKP, "keyframes": KEYFRAMES,
        "candidates_per_keyframe": CANDIDATES, "visible_per_frame": round(visible, 1),
        "matched_per_frame": round(matched, 1), "us": {k: round(v, 2) for k, v in us.items()},
        "cycle_us": round(cycle, 2), "cycle_le_observe": bool(cycle <= us["observe"]),
        "real_cull_died": died, "compact_kept": int(n_out.item())}), flush=True)
    return 0 if cycle <= us["observe"] else 1


if __name__ == "__main__":
    sys.exit(main())
