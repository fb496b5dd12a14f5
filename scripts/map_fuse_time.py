"""LandmarkMap.fuse beside LandmarkMap.observe in the same process.

At the tracking shape of scripts/map_life_time.py -- batch 32, 65,536 landmarks
in view plus 4,096 planted twins (1 cm off, 10 bits flipped), 2,087 keypoints
per 1280 x 720 frame -- the HIP-event time per call, launches included (200
back-to-back calls, median of 5), of observe, of its window search alone, of
slam_map_fuse and of slam_rows_fuse on one kept (rows, count).  A fuse kills
what it fuses, so every timed fuse is preceded by putting the map back; that
restore is timed alone as well.

At the shapes of the test scene (tests/test_map_life.py with the planted twins
of tests/test_map_fuse.py: batch 4, 1,024 slots, 448 keypoints) the time of
LandmarkMap.step with fuse=None and with fuse={}, the tracks forgotten after
every call so that the rewrite always sees one kept entry.  One JSON line.

    python scripts/map_fuse_time.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slam-1_amd"), os.path.join(ROOT, "scripts"),
                os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from slam355 import _lib, matcher  # noqa: E402
from slam355.device import ptr  # noqa: E402
from slam355.mapping import LandmarkMap  # noqa: E402

import guided_time as gt  # noqa: E402  (its scene, timer and shape: B, NKP, W, H, P)

M, TWINS = 65536, 4096
B, T = gt.B, gt.T


def tracking_shape(rng):
    X, D, poses, kp, desc = gt.scene(M, rng)
    d = rng.normal(size=(TWINS, 3))
    Xt = X[:TWINS] + 0.01 * d / np.linalg.norm(d, axis=1, keepdims=True)
    bits = np.unpackbits(D[:TWINS], axis=1)
    bits[:, :10] ^= 1
    lm = LandmarkMap(M + TWINS, gt.NKP, gt.W, gt.H, gt.P, cell=gt.CELL).add(
        np.r_[X, Xt], np.r_[D, np.packbits(bits, axis=1)])
    poses, kp, desc = T(poses), T(kp), T(desc)
    nt = torch.full((B,), gt.NKP, dtype=torch.int32, device=kp.device)

    def observe():
        out = lm.observe(0, poses, kp, desc, nt, radius=gt.RADIUS)
        lm.reset_tracks()
        return out

    rows, count = observe()
    b = lm._bufs[B]

    def window():
        matcher.window_knn2_batch(lm.desc, b["uv"], b["qr"], b["nq"], desc, kp, nt, b["grid"],
                                  out=(b["idx2"], b["dist2"], b["good0"]))

    state = [t.clone() for t in (lm.X, lm.visible, lm.found, lm.born, lm.last)]

    def restore():
        for t, t0 in zip((lm.X, lm.visible, lm.found, lm.born, lm.last), state):
            t.copy_(t0)

    def fuse():
        restore()
        lm.fuse(rewrite_tracks=False)

    fuse()
    torch.cuda.synchronize()
    nfused = int(lm.nfused.item())
    ws = lm._rows_fuse_ws(lm._fbufs[B], B)
    out = (torch.zeros_like(rows), torch.zeros_like(count))

    def rows_fuse():
        _lib.call("slam_rows_fuse", ptr(rows), ptr(count), int(rows.shape[1]), B, ptr(lm.to), lm.cap,
                  ptr(out[0]), ptr(out[1]), ptr(ws), ws.numel(), None)

    us = {"observe": gt.timed(observe), "window_knn2": gt.timed(window),
          "fuse_with_restore": gt.timed(fuse), "restore": gt.timed(restore),
          "rows_fuse": gt.timed(rows_fuse)}
    us["observe_again"] = gt.timed(observe)
    return {"landmarks": M + TWINS, "batch": B, "n_kp": gt.NKP, "fused": nfused,
            "rows_per_frame": round(float(count.sum()) / B, 1), "us": {k: round(v, 2) for k, v in us.items()}}


def scene_shape():
    import test_map_fuse as tf
    import test_map_life as tl

    s = tf._twin_scene()[0]
    args = tl._batch_args(s, 0)
    us = {"step": [], "step_fuse": []}
    for name, fuse in (("step", None), ("step_fuse", {})) * 3:   # alternating: the spread is in the lists
        lm = tf._twin_map()

        def call():
            lm.step(0, *args, z_range=tl.Z_RANGE, cull=tl.CULL, radius=tl.RADIUS, max_dist=tl.MAX_DIST,
                    ratio=tl.RATIO, fuse=fuse)
            lm.reset_tracks()

        us[name].append(round(gt.timed(call), 2))
    return {"slots": s["x_cap"], "batch": s["B"], "n_kp": s["cap"], "us": us,
            "ratio": round(float(np.median(us["step_fuse"]) / np.median(us["step"])), 4)}


def main():
    rng = np.random.default_rng(7)
    res = {"what": "map_fuse", "tracking_shape": tracking_shape(rng), "scene_shape": scene_shape()}
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
