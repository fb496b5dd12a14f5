"""The two 2-D compactions of the tracking front end on their own:
slam_compact_matches (compact_kernel) and slam_filter_pairs (k_filter_pairs) at
the tracking shape (batch 64, 2,087 entries per item: three chunks of the
1,024-lane workgroup) and at 16,384 entries per item (16 chunks) -- HIP-event
time per call, 200 back-to-back calls, median of 5.  One JSON line.

    python scripts/compact_time.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "slam-1_amd"), os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from slam355 import _lib  # noqa: E402
from slam355.device import ptr  # noqa: E402

import guided_time as gt  # noqa: E402  (its timer)

B = 64


def measure(n, rng):
    T = gt.T
    idx2 = T(rng.integers(0, n, (B, n, 2)).astype(np.int32))
    good = T((rng.random((B, n)) < 0.3).astype(np.uint8))       # the ratio test keeps about a third
    mask = T((rng.random((B, n)) < 0.8).astype(np.uint8))       # F-LMedS keeps most of those
    cnt = torch.full((B,), n, dtype=torch.int32, device="cuda")
    pairs = torch.zeros((B, n, 2), dtype=torch.int32, device="cuda")
    out = torch.zeros_like(pairs)
    c1, c2 = torch.zeros_like(cnt), torch.zeros_like(cnt)
    compact = lambda: _lib.call("slam_compact_matches", ptr(idx2), ptr(good), ptr(cnt), n, B, None,  # noqa: E731
                                0.0, ptr(pairs), ptr(c1), None)
    filt = lambda: _lib.call("slam_filter_pairs", ptr(idx2), ptr(cnt), ptr(mask), n, B, ptr(out),  # noqa: E731
                             ptr(c2), None)
    us = {"compact_matches": round(gt.timed(compact), 2), "filter_pairs": round(gt.timed(filt), 2)}
    assert int(c1.sum()) == int(good.sum()) and int(c2.sum()) == int(mask.sum())
    return us


def main():
    rng = np.random.default_rng(3)
    print(json.dumps({"what": "compact", "batch": B,
                      "us": {str(n): measure(n, rng) for n in (2087, 16384)}}), flush=True)


if __name__ == "__main__":
    main()
