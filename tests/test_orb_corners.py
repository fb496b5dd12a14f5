"""k_orb_tile's corner lists: the FAST drain appends every scored pixel inside
the NMS border to a wave-private list, and the NMS pass tests the list's entries
instead of scanning the score map for them.  A level in which some wave meets
more corners than its list holds scans the map as before; slam_orb_set_corner_cap
forces that on ordinary images.  Both paths must equal the CPU oracle bit for
bit (keypoints as uint32 views, octaves, descriptors) and each other.

Image sizes: 640x480 with the default tiling gives 96x144 patches, whose level-0
NMS region (34x82) holds ~700 corners of uniform noise (25 %), ~87 per wave: a
list of 64 overflows there, the default (174) does not, and levels >= 1 (<= 33
per wave) stay on the lists either way.  The 1280x720 frames (216x192 patches;
noise gives ~650 corners per wave on level 0, under the default 1251) run
levels 3-6 as the batched group.
"""
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu


def _dot_grid(H, W, step=10):
    img = np.zeros((H, W), np.uint8)
    for y in range(5, H - 5, step):
        img[y, 5:W - 5:step] = 255
    return img


@functools.lru_cache(maxsize=None)
def _images(name):
    if name == "mixed":  # dense noise, no corner at all, a few corners per wave (some waves none)
        noise = np.random.default_rng(7).integers(0, 256, (480, 640), dtype=np.uint8)
        return np.stack([noise, np.full((480, 640), 128, np.uint8), _dot_grid(480, 640)])
    if name == "odd":  # last tile row and column clipped by the image bounds
        return np.random.default_rng(11).integers(0, 256, (1, 301, 517), dtype=np.uint8)
    if name == "c2":
        from slam355.synthetic import stereo_sequence

        L, _, _, _ = stereo_sequence(2, seed=0)
        noise = np.random.default_rng(13).integers(0, 256, (1, 720, 1280), dtype=np.uint8)
        return np.concatenate([L, noise])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _expected(name, max_kp):
    return [oracle.orb_tiles(im, max_kp) for im in _images(name)]


def _run(name, max_kp, cap=0):
    import torch
    from slam355 import _lib, orb

    t = torch.from_numpy(_images(name)).cuda()
    try:
        _lib.call("slam_orb_set_corner_cap", cap)
        out = orb.orb_batch(t, max_kp, kp_cap=4096)  # (the dots' ties are all kept: 1247 at 14)
        torch.cuda.synchronize()
        out = [x.cpu().numpy().copy() for x in out]
    finally:
        _lib.call("slam_orb_set_corner_cap", 0)
    return out


def _check(out, name, max_kp):
    kp, octv, desc, cnt = out
    for b, (ek, eo, ed) in enumerate(_expected(name, max_kp)):
        n = cnt[b]
        assert n == len(ek), (b, n, len(ek))
        assert np.array_equal(kp[b, :n].view(np.uint32), ek.view(np.uint32)), b
        assert np.array_equal(octv[b, :n], eo), b
        assert np.array_equal(desc[b, :n], ed), b
    return cnt


def _same(a, b):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("max_kp", [14, 20])
def test_lists_with_remainder_and_empty_waves(max_kp):
    """One launch: lists far from a multiple of 64 (noise), every list empty
    (flat), fewer than 64 entries per wave and some waves with none (dots)."""
    cnt = _check(_run("mixed", max_kp), "mixed", max_kp)
    assert cnt[0] > 0 and cnt[1] == 0 and cnt[2] > 0


def test_border_and_clipped_tiles():
    """517x301 noise: corners on x = 31, W-32, y = 31, H-32 and just outside,
    in full and in clipped patches."""
    _check(_run("odd", 20), "odd", 20)


@pytest.mark.parametrize("name,max_kp", [("mixed", 14), ("odd", 20)])
def test_fallback_equals_lists(name, max_kp):
    """A cap of 64 entries per wave overflows on level 0 of the noise patches
    only: one launch mixes both paths.  Same arrays as the default, and the oracle's."""
    a, b = _run(name, max_kp), _run(name, max_kp, cap=64)
    _same(a, b)
    _check(a, name, max_kp)
    _check(b, name, max_kp)


def test_small_level_group_both_paths():
    """Two 1280x720 frames and one of noise, 64 kp per tile: levels 3-6 run as
    the batched group with one list per wave across its levels, and the noise's
    level 0 holds ten drains of 64 per wave; default cap and a cap of 64."""
    a, b = _run("c2", 64), _run("c2", 64, cap=64)
    assert (_check(a, "c2", 64) > 900).all()
    _check(b, "c2", 64)
    _same(a, b)
